// wx_align_dp.h — MI355X (gfx950 / CDNA4) kernel templates of WhisperX's forced-alignment DP,
// behind the C ABI of include/wx_align.h (host side and the non-template kernels:
// wx_align.hip; instantiations: the shards of wx_align_inst.hip).
//
// Reference being replaced (file:line in NADOOIT/whisperX @ 2025-01-12):
//   get_trellis    whisperx/alignment.py:359-379     -> trellis_kernel (materialising)
//   align() DP     whisperx/alignment.py:242-250     -> align_dp_kernel, align_dp_split_kernel
//                                                       (fused, no trellis) + walk
//   backtrack      whisperx/alignment.py:387-421     -> wx_align.hip: backtrack_kernel + walk
//   merge_repeats  whisperx/alignment.py:438-454     -> wx_align.hip: merge_repeats_kernel
//
// Design:
//   * One wave64 per segment.  The trellis recurrence is row-parallel: row t+1 depends only
//     on row t, so lane g owns the C contiguous cells j = g*C+1 .. g*C+C and a time step is
//     C independent add/add/max cells plus one DPP wave_shr:1 for the left neighbour of the
//     lane's first cell.  The sequential depth is T steps; throughput comes from many
//     segments (waves) in flight.
//   * Emission rows are staged 32 at a time into LDS (row stride VS = 32 or 64 floats) by
//     global_load_lds, double-buffered, so the per-cell gather em[t, tok[j-1]] is one
//     conflict-free ds_read_b32 with a compile-time immediate row offset.
//   * The fused kernel never writes the trellis.  The backtrack test at (t, j) is bit for
//     bit the forward comparison that produced trellis[t, j] (`changed > stayed`), so the
//     forward keeps one bit per cell per step: lane-local 32-step column words (v_cmp +
//     v_addc, shift-in), stored as [block][slot][lane].  The walk reads a 64-cell x 32-step
//     window of them per block into the wave's lanes and steps with v_readlane + scalar ops.
//   * merge_repeats is rebuilt from the walk's per-token start frames: token k spans
//     [start_k, start_{k+1}); its first frame carries exp(em[t, tok[k]]), the others
//     exp(em[t, 0]) (index 0, as alignment.py:409), summed left to right in fp64.
//
// Numerics are the reference's torch-CPU semantics (this file is compiled with
// -ffp-contract=off): fp32 adds, NaN-propagating max (v_maximum3_f32 == torch.maximum),
// strict `>` with ties staying, first-max/NaN-first argmax, fp64-accumulated column 0.
// One header per phase (wx_dp_config / prims / timing / forward / helpers / walk / tail .h,
// DESIGN.md §4.1); this one holds what joins them: the split arrival, align_dp_body, the kernels.
#ifndef WX_ALIGN_DP_H
#define WX_ALIGN_DP_H

#include "wx_dp_config.h"
#include "wx_dp_forward.h"
#include "wx_dp_helpers.h"
#include "wx_dp_prims.h"
#include "wx_dp_tail.h"
#include "wx_dp_timing.h"
#include "wx_dp_walk.h"
#include "wx_wave.h"  // kWave, lane_id, uniform*

namespace wx {

// Per-segment arrival of a split segment's parts.  The counter is one 8-byte word,
// {low: count | 0x80 if a part lost a hand-off, high: the launch's full 32-bit epoch}, so a
// word left by anything else never matches: a zeroed word has epoch 0 (never issued), an
// older launch's counter has an older epoch, and — the hand-off region being reused across
// batch layouts — an 8-byte hand-off granule that now sits where a counter lands carries
// its own launch's epoch in the same high half.  (Round 2 matched 24 epoch bits of a 4-byte
// word, which a granule's float half could match by chance.)  Returns the low word after
// this arrival.
// One round trip in the steady state: the CAS loop starts from a guessed word instead of a
// load — {epoch, part} for part > 0 (parts arrive in order when nothing is lost), the zero word
// for part 0 (the last part of the launch before reset the counter).  A wrong guess changes
// nothing: the CAS fails, returns the word that is there, and the loop goes on from it as it
// would from a load.
__device__ unsigned split_arrive(uint64_t* c, unsigned epoch, bool lost, int part) {
    uint64_t old = part > 0 ? (((uint64_t)epoch << 32) | (unsigned)part) : (uint64_t)0;
    while (true) {
        const unsigned cur = ((unsigned)(old >> 32) == epoch) ? (unsigned)old : 0u;
        const unsigned nw = ((cur & 0x7Fu) + 1u) | (cur & 0x80u) | (lost ? 0x80u : 0u);
        const uint64_t nv = ((uint64_t)epoch << 32) | nw;
        if (__hip_atomic_compare_exchange_strong(c, &old, nv, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return nw;
    }
}

// Latency buckets (H) claim more than half of a CU's 160 KB LDS so that the dispatcher
// places one workgroup per CU: two 8-wave workgroups on one CU would share its SIMDs
// (4 waves per SIMD) while other CUs idle.
constexpr int kLatencyLdsFloats = 84 * 1024 / 4;

// Column-map LDS of the gather (large-vocabulary) instantiations.
template <int VS>
struct ColMapLds {
    static constexpr bool kOn = VS == kGatherVS;
    unsigned bm[kOn ? kMaxVocabWords : 1];
    int wpre[kOn ? kMaxVocabWords + 1 : 1];
    int cols[kOn ? kGatherVS : 1];
};

// Build the segment's column map when VS is the gather width; returns false (and the
// caller stops) when the segment uses more distinct columns than a compact row holds.
template <int VS>
__device__ __forceinline__ bool prepare_colmap(ColMapLds<VS>& m, ColMap& cm, const int32_t* tok, int N, int blank,
                                               int V) {
    cm.bm = m.bm;
    cm.wpre = m.wpre;
    cm.cols = m.cols;
    cm.n = 0;
    if (!ColMapLds<VS>::kOn) return true;
    cm.n = build_colmap(tok, N, blank, V, m.bm, m.wpre, m.cols);
    return cm.n <= kGatherVS;
}

// Row slots of the checkpointed walk (CkSrc), [kChunk][VS] each: two per walker wave (the next
// block's rows load while a block computes) where that keeps the LDS of a workgroup within its
// share at 4 waves per SIMD (VS == 32, and the one-wave kernels' two forward buffers), else one
// per walker wave (rows loaded at use, the next block's warmed into the L2).
// (One slot per walker wave everywhere measured slower in round 5.)
template <int VS, int W>
constexpr int kCkSlots = (W == 1 || VS == 32) ? 2 * W : W;

// Split kernels: waves per workgroup.  Beyond the W DP waves and the two helpers, the rest
// only keep the forward's barrier count and then walk speculative segments (walk_spec: more
// walkers, shorter segments).  Eight, two per SIMD.  Registers no longer decide this: with the
// blank operand kept once per lane quad (Forward::RegOps) the DP waves' chunk code peaks at
// v126, and the kernel's 176 VGPRs are col0_helper's two sets of 32 doubles alone; with one
// set the register-resident kernels need 127 and twelve waves fit without a spill.  Built
// and measured in round 10: twelve waves (walk_spec's K = 11 on config 2)
// were 1.1 us slower than eight — every chunk barrier waits for twelve waves, and wave 0's
// chain through eleven walkers' records after the walk's barrier took back what the shorter
// segments gave.  (6 waves, no extra walkers: config 2 51.4 -> 53.3 us in round 5.)
constexpr int kSplitWaves = 8;
constexpr int kQ0LdsFrames = 4096;  // Split::q0l rows (longer segments: fill_q0 after the walk)

template <int C, int VS, int W, int H, bool SP = false, int XW = 0>
__device__ __forceinline__ void align_dp_body(const AlignArgs& a) {
    // Checkpointed forward (MODE 2, CkSrc walk): the single-CU throughput kernels with two or
    // more waves (speculative walkers) and staged row widths; the one-wave (a lone walker would
    // recompute every block serially: slower than the bits it saves), latency (helper), split
    // and gathered-vocabulary kernels keep the bitmap.
    constexpr bool CK = !SP && H == 0 && VS != kGatherVS && W >= 2;
    constexpr bool WT = split_wt<C, VS, SP>();  // write-through hand-over of the bits to the last part
    // (CK: the walkers' row slots, one [32][VS] per wave, reuse the forward's buffers)
    constexpr int kLdsFloats = H ? (kLatencyLdsFloats > 4 * kChunk * VS ? kLatencyLdsFloats : 4 * kChunk * VS)
                                 : (CK ? kCkSlots<VS, W> : 2) * kChunk * VS;
    __shared__ float lds[kLdsFloats];
    __shared__ __attribute__((aligned(16))) float c0b[H || (CK && W >= 2) ? 2 * kChunk : 1];
    __shared__ __attribute__((aligned(16))) float xh[W > 1 ? 2 * W * kWave : 1];
    __shared__ unsigned cmask_lds[kMaxLdsFrames / kChunk + 1];
    __shared__ int tsb[3];
    __shared__ int blo_lds;  // walk_tail: the walk's lowest block (-1: no path)
    __shared__ int colrec_lds[W + H > 1 ? kMaxLdsFrames / kChunk + 1 : 1];  // walk_spec records
    __shared__ int sbuf_lds[3 * (W + H + XW)];
    __shared__ ColMapLds<VS> cml;
    __shared__ float xg_lds[SP && C == 1 ? 2 * 32 : 1];  // Split::xg
    __shared__ float q0_lds[SP && XW > 0 ? kQ0LdsFrames : 1];  // Split::q0l
    const int P = SP ? a.parts : 1;
    // Split grids: block b = ((s / 8) * P + p) * 8 + s % 8, so the parts of segment s share
    // b % 8 — one XCD under the observed round-robin dispatch — and read its emission rows
    // through one L2.  (Placement is a speed matter only; part p - 1 has the lower block
    // index either way, so it starts no later than part p.)  kArgXcdSpread (tests) puts part p
    // at b % 8 = (s + p) % 8 instead: every part of a segment on another XCD.
    const int part = SP ? ((int)blockIdx.x / kXcdStride) % P : 0;
    const int xslot = (int)blockIdx.x % kXcdStride;
    const int seg = SP ? ((int)blockIdx.x / kXcdStride / P) * kXcdStride +
                             ((a.flags & kArgXcdSpread) ? (xslot - part) & (kXcdStride - 1) : xslot)
                       : (int)blockIdx.x;
    if (SP && seg >= a.S) return;  // grid padded to a multiple of 8 segments
    const SegDesc d = load_desc(a.em_off, a.tok_off, a.blank_id, seg);
    const int want = (SP || a.parts > 1) ? launch_split_bucket(d.N, a.parts, a.split_id) : bucket_id(d.N, a.mode);
    if (want != (bucket_make(C, W, H ? 1 : 0) | (SP ? kSplitFlag : 0))) return;  // another instantiation owns it
    const int lane = (int)threadIdx.x;
    if (d.N <= 0 || d.T <= 0) {
        if (lane == 0 && part == 0) {
            a.t_start[seg] = 0;
            a.status[seg] = 1;
        }
        return;
    }
    ColMap cm;
    // More than kGatherVS distinct columns: the compact LDS row cannot hold the segment's
    // emissions, so one workgroup (part 0 of a split) runs the generic forward instead.
    const bool slow = !prepare_colmap(cml, cm, a.tok + d.tok0, d.N, d.blank, a.V);
    if (slow && part != 0) return;
    const float* E = a.em + d.row0 * a.V;
    unsigned* bits = a.bits + ((d.row0 >> 5) + seg) * (int64_t)a.bits_stride_cells;
    float* q0 = a.q0 + d.row0;
    float* cn = a.cn + ((d.row0 + kCnPad * (int64_t)seg) & ~(int64_t)3);
    double* c0acc = a.c0acc + ((d.row0 >> 5) + seg);
    WX_STAMP_RT(4);
    WX_STAMP(0);
    Split sp;
    if (SP) {
        sp.p = part;
        sp.P = P;
        sp.lanes = kWave * W * P;
        sp.tag = a.epoch;
        sp.xstride = (kMaxParts - 1) * kHaloCells;
        sp.spin = a.spin;
        uint64_t* xseg = a.xg + ((d.row0 >> 5) + seg) * (int64_t)sp.xstride;
        sp.xin = xseg + (part > 0 ? part - 1 : 0) * kHaloCells;
        sp.xout = xseg + part * kHaloCells;
        sp.xg = xg_lds;
        sp.q0l = (XW > 0 && d.T <= kQ0LdsFrames) ? q0_lds : nullptr;
    }
    if (SP && lane == 0) tsb[2] = 0;
    bool lost = false;
    if (!slow)
        lost = Forward<C, VS, CK ? 2 : 0, W, H != 0, SP, (H > 1 ? 2 : 1)>::run(
            d, E, a.V, a.tok, bits, q0, cn, nullptr, lds, c0b, xh, a.x4 != 0, cm, nullptr, &sp, c0acc);
    WX_STAMP(1);
    if (SP && lost) tsb[2] = 1;  // (any lane of the consumer or, register-resident kernels, the poller)
    wait_vm();
    block_fence();
    bool failed = false;
    if (SP && !slow) {  // release this part's bits / column-N history; the last part to arrive goes on
        if (lane == 0) {
            // (WT: every wave's stores drained above, then the barrier: no release)
            const bool fenced = !WT || (a.flags & kArgFenced);
            if (fenced) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                wait_vm();
            }
            const unsigned w = split_arrive(a.arrive + seg, a.epoch, tsb[2] != 0, part);
            tsb[0] = ((w & 0x7Fu) == (unsigned)P) ? 1 + (int)((w >> 7) & 1u) : 0;
            if (tsb[0]) {
                if (fenced) {  // (WT: the walk reads the parts' words with sc1 loads)
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    wait_vm();
                }
                // every part has arrived: leave the counter clean for the next launch
                __hip_atomic_store(a.arrive + seg, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        if (tsb[0] == 0) {
            WX_STAMP(2);
            WX_STAMP(3);
            WX_STAMP_RT(5);
            return;
        }
        failed = tsb[0] == 2;
        __syncthreads();
    }
    const Layout lay = Layout::make(C, d.N, kWave * W * P);
    if (slow || failed) {
        // recovery: a lost hand-off (some part computed with a stale halo) or a segment whose
        // columns do not fit the compact row.  The whole workgroup recomputes the segment.
        if (!generic_forward(d.T, d.N, d.blank, E, a.V, a.tok + d.tok0, bits, lay, cn, q0, lds, kLdsFloats)) {
            if (lane == 0) {
                a.t_start[seg] = 0;
                a.status[seg] = slow ? 2 : 3;  // (N too large for the generic forward's LDS rows)
            }
            return;
        }
        wait_vm();
        block_fence();
    }
    int32_t* start = a.seg_start + d.tok0;
    WX_T(w0);
    // t_start, the walk and the change masks: several waves walk speculative segments, one per
    // wave (walk_spec, which also finds t_start); one wave walks alone
    const int nbw = ((d.T - 1) >> 5) + 1;
    const bool lds_walk = d.T <= kMaxLdsFrames;
    // q0 already in this workgroup's LDS (Split::q0l; the recovery paths write it to q0)
    const bool q0l_ok = SP && XW > 0 && d.T <= kQ0LdsFrames && !slow && !failed;
    const int K = lds_walk ? max(1, min(W + H + XW, nbw / kSpecMinBlocks)) : 1;
    WX_T(w1);
    WX_TDECL(w2 = 0);
    auto walk_tail = [&](auto& wsrc) {
    int ts = 0, b_lo = -1;
    unsigned* cmask = lds_walk ? cmask_lds : a.cmask + ((d.row0 >> 5) + seg);
    if constexpr (W + H > 1) b_lo = walk_spec(wsrc, d.N, d.T, cn, cmask, lds_walk, K, colrec_lds, sbuf_lds, ts);
    if (lane < kWave) {  // wave 0: t_start, the walk, then the change masks -> start frames
        if constexpr (W + H == 1) {
            ts = column_argmax<WT>(cn, d.T);
            b_lo = walk_impl(wsrc, d.N, ts, cmask, lds_walk);
        }
        if (lane == 0) {
            a.t_start[seg] = ts;
            tsb[0] = ts;
        }
        WX_TSET(w2);
        if (!H && b_lo >= 0) {
            wave_fence();
            compact_starts(cmask, b_lo, (ts - 1) >> 5, start);
        }
        if (lane == 0) {
            tsb[1] = b_lo >= 0 ? 1 : 0;
            blo_lds = b_lo;
        }
    } else {
        if (H && !slow && !failed && !q0l_ok) fill_q0(E, a.V, d.T, q0, kWave);
    }
    if constexpr (H != 0) {  // latency / split kernels: the compaction over every wave
        block_fence();  // (wave 0's change masks, b_lo, t_start)
        const int bl = uniform(blo_lds);
        if (bl >= 0) compact_starts_par(cmask, bl, (uniform(tsb[0]) - 1) >> 5, start);
    }
    WX_T(w3);
    WX_TDUMP(lane == 0, 15, w1 - w0, w2 - w1, w3 - w2);  // walk-phase split: argmax, walk, compaction
    };
    if constexpr (CK) {
        CkSrc<C, VS> wsrc;
        wsrc.ck = reinterpret_cast<const float*>(bits);
        wsrc.lay = lay;
        wsrc.acc = c0acc;
        wsrc.E = E;
        wsrc.tok = a.tok + d.tok0;
        wsrc.T = d.T;
        wsrc.N = d.N;
        wsrc.V = a.V;
        wsrc.blank = d.blank;  // (as the forward reads it)
        wsrc.x4 = a.x4 != 0;
        // one-wave kernels: both forward buffers are the walker's two slots; else one per wave
        wsrc.slot[0] = lds + uniform((int)threadIdx.x >> 6) * kChunk * VS;
        wsrc.slot[1] = kCkSlots<VS, W> >= 2 * W ? wsrc.slot[0] + W * kChunk * VS : wsrc.slot[0];
        wsrc.junk = xh;  // (the forward's halo exchange, free now: 2 W 64 floats >= 1 KB when W > 1)
        walk_tail(wsrc);
    } else {
        BitSrc<C, WT> wsrc{bits, lay};
        walk_tail(wsrc);
    }
    wait_vm();
    block_fence();
    const int ts = tsb[0];
    const bool ok = tsb[1] != 0;
    WX_STAMP(2);
    // low bits: 0 aligned / 1 None; flags: which segments took the generic forward
    if (lane == 0) a.status[seg] = (ok ? 0 : 1) | (failed ? WX_STATUS_RECOVERED : 0) | (slow ? WX_STATUS_GENERIC : 0);
    if (!ok) return;
    // (staging costs one more round trip: it pays when every thread has several tokens)
    if (d.T + d.N <= kLdsFloats && d.N > 2 * (int)blockDim.x)
        merge_tokens_lds(E, a.V, a.tok + d.tok0, d.N, d.T, ts, q0l_ok ? q0_lds : q0, start, a.seg_end + d.tok0,
                         a.seg_score + d.tok0, lds);
    else
        merge_tokens(E, a.V, a.tok + d.tok0, d.N, ts, q0l_ok ? q0_lds : q0, start, a.seg_end + d.tok0,
                     a.seg_score + d.tok0);
    WX_STAMP(3);
    WX_STAMP_RT(5);
}

template <int C, int VS, int W, int H>
__global__ __launch_bounds__(kWave*(W + H)) __attribute__((amdgpu_waves_per_eu(H || VS == kGatherVS || C > 8 || W == 1 ? 1 : 4, H ? 2 : 8))) void align_dp_kernel(
    AlignArgs a) {
    align_dp_body<C, VS, W, H>(a);
}

// Split segments: P workgroups (parts, one per CU) per segment, grid = ceil(S / 8) * 8 * P.
template <int C, int VS, int W>
__global__ __launch_bounds__(kWave * kSplitWaves) __attribute__((amdgpu_waves_per_eu(1, 2))) void align_dp_split_kernel(
    AlignArgs a) {
    static_assert(W + 2 <= kSplitWaves && kSplitWaves <= 8, "split workgroup: W DP waves + 2 helpers + walkers");
    align_dp_body<C, VS, W, 2, true, kSplitWaves - W - 2>(a);
}

template <int C, int VS, int W>
__global__ __launch_bounds__(kWave * W) void trellis_kernel(TrellisArgs a) {
    __shared__ float lds[2 * kChunk * VS];
    __shared__ float xh[W > 1 ? 2 * W * kWave : 1];
    __shared__ ColMapLds<VS> cml;
    __shared__ __attribute__((aligned(16))) float rst[W * kWave * C];
    const int seg = blockIdx.x;
    const SegDesc d = load_desc(a.em_off, a.tok_off, a.blank_id, seg);
    if (bucket_id(d.N) != bucket_make(C, W, 0)) return;
    float* tr = a.tr + a.tr_off[seg];
    const int lane = (int)threadIdx.x;
    if (d.N == 0) {  // the whole single column is +inf (alignment.py:369-370 with num_tokens = 0)
        for (int t = lane; t <= d.T; t += kWave * W) tr[t] = INFINITY;
        return;
    }
    ColMap cm;
    if (!prepare_colmap(cml, cm, a.tok + d.tok0, d.N, d.blank, a.V)) {  // too many distinct columns
        const int64_t n = (int64_t)(d.T + 1) * (d.N + 1);
        for (int64_t i = lane; i < n; i += kWave * W) tr[i] = NAN;
        return;
    }
    const float* E = a.em + d.row0 * a.V;
    Forward<C, VS, 1, W, false>::run(d, E, a.V, a.tok, nullptr, nullptr, nullptr, tr, lds, nullptr, xh, a.x4 != 0,
                                     cm, rst);
}

}  // namespace wx

#endif  // WX_ALIGN_DP_H
