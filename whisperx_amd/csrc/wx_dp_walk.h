// wx_dp_walk.h — the backtrack of the alignment DP (wx_align_dp.h, and wx_align.hip's backtrack_kernel):
// column N's argmax, the (speculative) walk over decision words, change masks -> start frames.
#ifndef WX_DP_WALK_H
#define WX_DP_WALK_H

#include "wx_dp_config.h"  // kChunk, Layout
#include "wx_dp_prims.h"
#include "wx_dp_timing.h"  // WX_T, WX_TACC, WX_TDUMP
#include "wx_wave.h"

namespace wx {

// Argmax of column N over rows 0..T with torch.argmax semantics (first maximum; the first
// NaN wins), rows 1..T read from cn[0..T-1], row 0 = -inf (alignment.py:395-396).  Wave 0.
template <bool WT = false>  // WT: sc1 loads (a split segment's history, written through by another CU)
__device__ int column_argmax(const float* __restrict__ cn, int T) {
    const int l = lane_id();
    int nan_row = 0x7fffffff, best_row = 0;
    float best = -INFINITY;
    // loads in flight per lane.  WT: the history was written through, so every load goes out
    // to the fabric (~1 us): one round for T <= 2048 (8 per lane took 3 rounds at T = 1499)
    constexpr int kBatch = WT ? 32 : 8;
    for (int base = 0; base < T; base += kBatch * kWave) {
        float v[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {  // (unconditional, clamped: no wait at the issue)
            const int i = base + u * kWave + l;
            v[u] = ld_pub<WT>(cn + min(i, T - 1));
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u)
            if (base + u * kWave + l >= T) v[u] = -INFINITY;
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {  // rows of a lane in increasing order
            const int row = base + u * kWave + l + 1;
            if (v[u] != v[u]) {
                nan_row = min(nan_row, row);
            } else if (v[u] > best) {
                best = v[u];
                best_row = row;
            }
        }
    }
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        nan_row = min(nan_row, __shfl_xor(nan_row, off));
        const float b2 = __shfl_xor(best, off);
        const int r2 = __shfl_xor(best_row, off);
        if (b2 > best || (b2 == best && r2 < best_row)) {
            best = b2;
            best_row = r2;
        }
    }
    return uniform(nan_row != 0x7fffffff ? nan_row : best_row);
}

// ------------------------------------------------------------------------------------
// Backtrack walk over the decision bitmap (alignment.py:395-421).  Uniform control flow,
// executed by the whole wave; `lay` maps cells to the bitmap's (lane, slot) words.
// Records start[k] = first frame of token k (the frame where the path moved onto it).
// Returns true on success (j reached 0), false where the reference returns None.
template <int CC, bool WT = false>  // WT: sc1 loads (kSplitWT)
__device__ __forceinline__ unsigned load_window(const unsigned* __restrict__ bits, const Layout& lay, int b, int A) {
    // Unconditional (column clamped to 1, block to 0): the walk masks invalid lanes when it
    // uses the word, so the load can stay in flight across blocks (a conditional load
    // merges into its destination and hipcc then waits for it where it is issued).
    // The block's row base is wave-uniform (scalar 64-bit math); the lane adds a 32-bit word
    // offset, so the load takes the saddr + voffset form with no per-lane 64-bit multiply.
    const unsigned* row = bits + (int64_t)uniform(max(b, 0)) * (lay.C * lay.lanes);
    const int jj = max(A - lane_id(), 1);
    int g, k;
    lay.locate<CC>(jj - 1, g, k);
    return ld_pub<WT>(row + (unsigned)(k * lay.lanes + g));
}

// Walk one 32-step block (decision indices 32b+31 .. 32b) from window offset d, run-length
// form: one iteration per token change instead of per step.  The path stays on window lane
// d until the next set bit (in walking order: increasing bit position) of that lane's word,
// moves there, and continues from the next step on lane d+1.  A successful path makes
// exactly N changes, so the serial chain costs ~N * (readlane + 8 SALU) per segment instead
// of T * 4 SALU (a per-step ballot-transposed SALU chain, replaced in round 2).  Bits of
// steps before the walk's start must be cleared.  Returns the change mask (bit 31-s = the
// path moved onto a new token at 32b+s).
__device__ __forceinline__ unsigned walk_block_rl(unsigned win, int& d) {
    // Per change: x = word[dd] & m (m: bit positions still ahead) is non-zero; p = its lowest
    // set bit is the change; m = -2 << p keeps the positions after it (0 after bit 31: the
    // walk leaves the block).  The chain is s_and -> s_ff1 -> s_lshl; the next lane's word
    // (dd does not depend on the chain) is read one change ahead so v_readlane stays off
    // it (lane dd + 1 may be past the window: read, never used).  Unrolled by four: a taken
    // branch costs more than the rest of a change (measured ~96 cycles per change for the
    // loop with one taken branch per change).
    // The lane position is not carried through the chain: every change sets one bit of cm, so
    // the walk leaves the block on lane d + popcount(cm).  Words are read two changes ahead
    // (wa / wb alternate), which keeps v_readlane's SGPR write two changes off its reader.
    unsigned cm = 0u, m = 0xFFFFFFFFu, x, wa, wb, t = (unsigned)d + 2u, p;
#define WX_RL_STEP(W, BR)                       \
    "s_ff1_i32_b32 %[p], %[x]\n\t"              \
    "s_bitset1_b32 %[cm], %[p]\n\t"             \
    "s_lshl_b32 %[m], -2, %[p]\n\t"             \
    "s_add_u32 %[t], %[t], 1\n\t"               \
    "s_and_b32 %[x], %[" #W "], %[m]\n\t"       \
    "v_readlane_b32 %[" #W "], %[win], %[t]\n\t" BR "\n\t"
    asm volatile(
        "s_add_u32 %[p], %[t], -2\n\t"
        "v_readlane_b32 %[x], %[win], %[p]\n\t"
        "s_add_u32 %[p], %[t], -1\n\t"
        "v_readlane_b32 %[wa], %[win], %[p]\n\t"
        "v_readlane_b32 %[wb], %[win], %[t]\n\t"
        "s_and_b32 %[x], %[x], %[m]\n\t"
        "s_cbranch_scc0 2f\n"
        "1:\n\t"
        WX_RL_STEP(wa, "s_cbranch_scc0 2f")
        WX_RL_STEP(wb, "s_cbranch_scc0 2f")
        WX_RL_STEP(wa, "s_cbranch_scc0 2f")
        WX_RL_STEP(wb, "s_cbranch_scc1 1b")
        "2:"
        : [t] "+s"(t), [cm] "+s"(cm), [m] "+s"(m), [x] "=&s"(x), [wa] "=&s"(wa), [wb] "=&s"(wb), [p] "=&s"(p)
        : [win] "v"(win)
        : "scc");
#undef WX_RL_STEP
    d += __popc(cm);
    return cm;
}

// Speculative walk segments (multi-wave workgroups, T <= kMaxLdsFrames).  The blocks below the
// top are cut into K segments of L blocks; the walker wave of segment k >= 1 starts at its top
// block from a guessed column and records its column after every block (colrec), its result
// and its end column.  Backtrack paths from different cells merge (Viterbi survivor paths),
// and the walk is a function of (block, column) alone, so once the true walk (wave 0) stands
// where segment k's walker stood after the same block — or enters segment k on its guessed
// column — the rest of that segment's change masks, end column and result are the true
// walk's, and wave 0 jumps to the segment's end.
// Decision words from the forward's bitmap (load_window): block bb's window issued at column
// A holds columns A - lane (lo) and A - 64 - lane (hi); at use the 64 lanes from the walk's
// offset are gathered (two ds_bpermutes, skipped while the block fits the first word).
template <int CC, bool WT = false>  // WT: the words were written through by other CUs (kSplitWT)
struct BitSrc {
    static constexpr bool kWT = WT;
    const unsigned* bits;
    Layout lay;
    struct Win {
        unsigned lo, hi;
        int A;
    };
    __device__ __forceinline__ void issue(Win& w, int bb, int A) const {
        w.A = uniform(A);
        w.lo = load_window<CC, WT>(bits, lay, bb, A);
        w.hi = load_window<CC, WT>(bits, lay, bb, A - 64);
    }
    __device__ __forceinline__ void end_block(int) const {}
    __device__ __forceinline__ void window(const Win& w, int b, int j, unsigned& win, int& dd) const {
        (void)b;
        const int lane = lane_id();
        const int d = uniform(w.A - j);  // 0 .. 96
        if (d <= 31) {
            win = (w.A - lane >= 1) ? w.lo : 0u;
            dd = d;
        } else {
            const int o = d + lane;  // column w.A - o
            const unsigned a = (unsigned)__shfl((int)w.lo, o & 63);
            const unsigned h = (unsigned)__shfl((int)w.hi, o & 63);
            win = (w.A - o >= 1 && o < 128) ? (o < 64 ? a : h) : 0u;
            dd = 0;
        }
    }
};

// Decision words recomputed from checkpoint rows (MODE 2 kernels).  The backtrack test at
// (t, j) is the forward's comparison `tr[t-1, j-1] + em[t-1, tok[j-1]] > tr[t-1, j] + em[t-1,
// blank]` (alignment.py:372-378, :400-404), and fp32 adds and maxima are deterministic, so the
// forward's decisions are recomputed bit for bit from the row it started the chunk with.  A
// block's path enters at column j and leaves at >= j - 32, so its words are needed for columns
// j - 32 .. j; over 32 steps a cell depends on the 32 cells to its left, so the band is the
// 64 lanes L -> column j - 63 + L started from checkpoint row 32b plus column j - 64 as lane 0's
// first left input: lane L's decision at step k is exact when L >= k (lane 0's later left
// inputs are unknown), i.e. columns >= j - 32 at every step.  Column 0 (tr[t][0], :367-370)
// is not a cell: where the band reaches it, its lane is set every step from the fp64 cumsum
// (checkpointed per chunk) in the reference's order.
//
// The block's 32 emission rows are staged per wave into an LDS slot ([32][VS], row stride VS
// so the per-step reads take immediate offsets) by LDS-DMA.  A walker with two slots (one-wave
// kernels: the forward's two buffers) loads the next block's rows into the other slot while it
// computes; one slot per walker (multi-wave kernels) loads its rows at use and warms the L2
// with the next block's rows (a DMA into a shared scratch row nobody reads).  The checkpoint
// values and token ids of the window are loaded with the walk's three-block prefetch (columns
// A - lane, A - 64 - lane, A - 128 - lane: the band of a block entered within 96 columns of A).
template <int CC, int VS>
struct CkSrc {
    static constexpr bool kWT = false;
    const float* ck;      // checkpoint rows: tr[32q][j] at cell j's bitmap word of block q
    Layout lay;
    const double* acc;    // [q]: sum of em[0 .. 32q - 1, 0] in fp64 (column 0 before row 32q)
    const float* E;       // segment's emission rows [T, V]
    const int32_t* tok;   // segment's tokens
    int T, N, V, blank;
    bool x4;              // V == 32 and 16-byte aligned rows: 8 rows per DMA instruction
    float* slot[2];       // LDS [kChunk][VS] slots of this wave (slot[1] == slot[0]: one slot)
    float* junk;          // LDS: 1 KB the L2 warm-up DMA writes
    int cur = 0, rdy_blk = -1000;  // slot holding block rdy_blk's rows, landed
    struct Win {
        float c0, c1, c2;  // checkpoint row of block bb: columns A - lane, A - 64 - lane, A - 128 - lane
        int k0, k1, k2;    // token ids of the same columns
        int A;
    };
    __device__ __forceinline__ float ck_of(const float* row, int col) const {
        col = max(col, 1);  // (columns <= 0: a don't-care lane)
        int g, k;
        lay.locate<CC>(col - 1, g, k);
        return row[(unsigned)(k * lay.lanes + g)];
    }
    __device__ __forceinline__ int tok_of(int col) const { return tok[max(col, 1) - 1]; }
    __device__ __forceinline__ void issue(Win& w, int bb, int A) const {
        w.A = uniform(A);
        const int lane = lane_id();
        const int bc = uniform(max(bb, 0));
        const float* row = ck + (int64_t)bc * (lay.C * lay.lanes);
        w.c0 = ck_of(row, A - lane);
        w.c1 = ck_of(row, A - 64 - lane);
        w.c2 = ck_of(row, A - 128 - lane);
        w.k0 = tok_of(A - lane);
        w.k1 = tok_of(A - 64 - lane);
        w.k2 = tok_of(A - 128 - lane);
    }
    // LDS-DMA of block b's rows (clamped into the segment) to dst, or all onto the junk row
    __device__ __forceinline__ void dma_rows(int b, float* dst, bool warm) const {
        const int l = lane_id();
        const int r0 = max(b, 0) * kChunk;
        const unsigned base = (unsigned)uniform((int)lds_addr(warm ? junk : dst));
        if (VS == 32 && x4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = min(r0 + 8 * i + (l >> 3), T - 1);
                glds_dwordx4(E, (unsigned)(r * 32 + (l & 7) * 4) * 4u, base + (warm ? 0u : (unsigned)(i * 1024)));
            }
        } else if (l < V) {
            for (int r = 0; r < kChunk; ++r) {
                const int t = min(r0 + r, T - 1);
                glds_dword(E + (int64_t)t * V, (unsigned)l * 4u, base + (warm ? 0u : (unsigned)(r * VS * 4)));
            }
        }
    }
    // The slot holding block b's rows.  Two slots: block b - 1's rows go into the other slot now
    // and are waited for at the end of block b (end_block), a block later.  One slot: the L2 is
    // warmed with block b - 1's rows now; end_block loads them into the slot once block b's
    // recompute has read it.  (Waiting for a DMA here would also wait for the window loads the
    // walk issued at the end of the previous block: an HBM round trip per block.)
    __device__ __forceinline__ const float* stage(int b) {
        const bool two = slot[1] != slot[0];
        if (uniform(rdy_blk) != b) {  // (the first block, or after a jump)
            cur = 0;
            dma_rows(b, slot[0], false);
            wait_vm();
            rdy_blk = b;
        }
        const float* s = cur ? slot[1] : slot[0];  // (no dynamic index: it would put the struct in scratch)
        if (two)
            dma_rows(b - 1, cur ? slot[0] : slot[1], false);
        else
            dma_rows(b - 1, nullptr, true);
        return s;
    }
    // block b walked: the next block's rows ready before the walk issues its next window loads
    __device__ __forceinline__ void end_block(int b) {
        if (slot[1] != slot[0]) {
            wait_vm();
            cur ^= 1;
        } else {
            dma_rows(b - 1, slot[0], false);
            wait_vm();
        }
        rdy_blk = b - 1;
    }
    __device__ __forceinline__ void window(const Win& w, int b, int j, unsigned& win, int& dd) {
        const int lane = lane_id();
        const int d = uniform(w.A - j);  // 0 .. 96
        const float* slotp = stage(b);
        // band lane L: column j - 63 + L, at window offset o = d + 63 - L
        const int o = d + 63 - lane;
        const float x0 = __shfl(w.c0, o & 63), x1 = __shfl(w.c1, o & 63), x2 = __shfl(w.c2, o & 63);
        const int y0 = __shfl(w.k0, o & 63), y1 = __shfl(w.k1, o & 63), y2 = __shfl(w.k2, o & 63);
        float v = o < 64 ? x0 : (o < 128 ? x1 : x2);
        int tk = o < 64 ? y0 : (o < 128 ? y1 : y2);
        tk = (tk >= 0 && tk < V) ? tk : 0;
        const int o0 = d + 64;  // column j - 64: lane 0's first left input
        // (column 0 when j == 64: not a checkpointed cell)
        const float left0 = j == 64 ? col0_value(b * kChunk, acc[max(b, 0)], T, N)
                                    : uniformf(o0 < 128 ? __shfl(w.c1, o0 & 63) : __shfl(w.c2, o0 & 63));
        const char* sb = reinterpret_cast<const char*>(slotp);
        const int toff = tk * 4, boff = blank * 4;
        unsigned bits = 0u;
        // 32 steps in groups of four, the next group's LDS operands read ahead (sched_barrier
        // keeps hipcc from hoisting all the reads: registers are the forward's occupancy).
        // HAS_C0: column 0 is band lane 63 - j (j <= 63), set every step from the cumsum.
        auto steps = [&](auto has_c0_tag) {
            constexpr bool HAS_C0 = decltype(has_c0_tag)::value;
            const bool c0 = HAS_C0 && lane == 63 - j;
            double a = HAS_C0 ? acc[max(b, 0)] : 0.0;  // (rare: a load in the chain is fine)
            const int t0 = b * kChunk;
            if (c0) v = col0_value(t0, a, T, N);
            float eb[4], et[4], e0[4];
            auto rd = [&](int k0, float(&xb)[4], float(&xt)[4], float(&x0)[4]) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    xb[u] = *reinterpret_cast<const float*>(sb + boff + (k0 + u) * VS * 4);
                    xt[u] = *reinterpret_cast<const float*>(sb + toff + (k0 + u) * VS * 4);
                    if (HAS_C0) x0[u] = *reinterpret_cast<const float*>(sb + (k0 + u) * VS * 4);
                }
            };
            rd(0, eb, et, e0);
#pragma unroll
            for (int g = 0; g < kChunk / 4; ++g) {
                float nb[4], nt[4], n0[4];
                if (g + 1 < kChunk / 4) rd(4 * (g + 1), nb, nt, n0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = 4 * g + u;
                    const float left = k == 0 ? dpp_shr1(left0, v)
                                              : __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
                                                                              __builtin_bit_cast(int, v), 0x138 /* wave_shr:1 */,
                                                                              0xF, 0xF, true));
                    const float st = v + eb[u];
                    const float ch = left + et[u];
                    bits = shift_in(bits, ch, st);
                    v = nan_max(st, ch);
                    if constexpr (HAS_C0) {
                        a += (double)e0[u];
                        if (c0) v = col0_value(t0 + k + 1, a, T, N);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    eb[u] = nb[u];
                    et[u] = nt[u];
                    if (HAS_C0) e0[u] = n0[u];
                }
            }
        };
        if (j > 63)
            steps(BoolTag<false>{});
        else
            steps(BoolTag<true>{});
        // lane i of the walk's window = column j - i = band lane 63 - i
        const unsigned r = (unsigned)__shfl((int)bits, 63 - lane);
        win = (j - lane >= 1) ? r : 0u;
        dd = 0;
    }
};

struct SpecWalk {
    int K, L0, Lb, ex, top;  // segments; blocks of segment 0 (L0), of the others (Lb, +1 for k <= ex)
    const int* colrec;  // LDS, per block: the segment walker's column after it (-1: not reached)
    const int* gstart;  // LDS [K]: guessed column at the top of segment k
    const int* sres;    // LDS [K]: the walker's result (-2: the path continues below the segment)
    const int* send;    // LDS [K]: its column after the segment's last block
    // after the barrier: gstart / sres / send of segment `lane` in lane `lane` (read by
    // v_readlane: the merge chain was a serial LDS round trip per segment)
    int vg, vr, ve;
    __device__ __forceinline__ int gst(int k) const { return __builtin_amdgcn_readlane(vg, k); }
    __device__ __forceinline__ int res(int k) const { return __builtin_amdgcn_readlane(vr, k); }
    __device__ __forceinline__ int end(int k) const { return __builtin_amdgcn_readlane(ve, k); }
    // segment k covers blocks lo(k) .. lo(k - 1) - 1 (segment 0: up to top); lo(K - 1) = 0
    __device__ __forceinline__ int lo(int k) const {
        return k == 0 ? top - L0 + 1 : max(top - L0 - (k * Lb + min(k, ex)) + 1, 0);
    }
};

// The backtrack walk (alignment.py:395-421) over the decision bitmap: from column j at the
// top of block b (steps above the start cleared by first_mask), step back one frame at a time
// and move to the previous token where the decision bit is set.  Once j reaches 0 the window
// reads cell 0 (all zero), so blocks run to completion without an early-exit test.  Per
// block only the change mask is kept (cmask[b]); start frames are compacted from it
// afterwards.  Returns the block where j reached 0, -1 where the reference returns None
// (block 0 done with j > 0), or -2 when it stopped after block b_stop > 0 with the path
// going on (column in j_out).  colrec (LDS, optional) receives the column after each block;
// spec (optional) lets the walk jump over blocks a merged segment walker has done.
//
// The bitmap words are global loads (written by other waves or CUs), so the walk keeps three
// blocks' windows in flight: the window of block b - 3 is issued when block b starts, at the
// column A the walk has then; lane i loads the words of columns A - i and A - 64 - i.  The
// path moves at most 32 columns per block, so block b - 3 starts at most 64 columns left of
// A and ends within 128 of it.  At use, the 64 lanes from the walk's offset are gathered
// into one word per lane (two ds_bpermutes, skipped while the block fits the first word).
//
// Src is where the decision words come from: BitSrc reads the forward's bitmap, CkSrc (the
// checkpointed throughput kernels) recomputes each block's band from the forward's checkpoint
// rows.  Src::issue(w, bb, A) starts block bb's loads for a walk standing at column A;
// Src::window(w, b, j, win, dd) makes win = the block's words with lane dd + i = column j - i.
template <class Src>
__device__ __forceinline__ int walk_range(Src& src, int j, int b, unsigned first_mask, int b_stop,
                                          unsigned* cmask, bool cmask_in_lds, int* colrec, const SpecWalk* spec,
                                          int& j_out, int wtop = 0x7fffffff, int* jentry = nullptr) {
    using Win = typename Src::Win;
    typedef __attribute__((address_space(3))) int lds_int;
    const int lane = lane_id();
    b = uniform(b);
    j = uniform(j);
    WX_TDECL(t_rl = 0, n_ch = 0, n_bl = 0, t_win = 0);
    auto dump = [&]() {  // (timing build: the walk's counters on its way out)
        WX_TDUMP(threadIdx.x == 0, 13, t_rl, n_ch, n_bl);  // (wave 0's last walk_range)
        WX_TDUMP((threadIdx.x & 63) == 0 && ((int)threadIdx.x >> 6) < 8, (spec ? 24 : 16 + ((int)threadIdx.x >> 6)),
                 t_win, t_rl, n_bl);
    };
    unsigned cmv = 0u;    // change masks of blocks gb + lane
    int gtop = b & 63;    // highest lane of the current group the walk has written
    int sk = 0, slo = spec ? spec->lo(0) : 0;  // segment of the current block, its lowest block
    auto flush = [&](int bb) {  // store the group's masks written since the last flush (blocks >= bb)
        const int gb = bb & ~63;
        if (lane >= (bb & 63) && lane <= gtop && gb + lane <= wtop) {
            if (cmask_in_lds)
                ((__attribute__((address_space(3))) unsigned*)cmask)[gb + lane] = cmv;
            else
                ((__attribute__((address_space(1))) unsigned*)cmask)[gb + lane] = cmv;
        }
        gtop = 63;
    };
    auto issue = [&](Win& w, int bb, int A) { src.issue(w, bb, A); };
    // walks block b with window w (wn, wa: the next two blocks' windows, re-issued after a
    // jump); false when the walk is over (result in res)
    auto block = [&](Win& w, Win& wn, Win& wa, int& res) -> bool {
        unsigned win;
        int dd;
        WX_T(wi0);
        src.window(w, b, j, win, dd);
        win &= first_mask;
        WX_TONLY(asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"));  // (the gather's loads, timed)
        WX_T(wi1);
        WX_TACC(t_win, wi1 - wi0);
        first_mask = 0xFFFFFFFFu;
        const int d0 = dd;
        WX_T(rl0);
        const unsigned cm = walk_block_rl(win, dd);
        WX_T(rl1);
        WX_TACC(t_rl, rl1 - rl0);
        WX_TACC(n_ch, __popc(cm));
        WX_TACC(n_bl, 1);
        // change masks are collected in lane b % 64 and stored 64 blocks at a time, through
        // an explicit LDS or global store (a flat store in the loop makes hipcc drain every
        // pending load at each wait)
        cmv = lane == (b & 63) ? cm : cmv;
        j = uniform(j - (dd - d0));
        if (b > wtop) {  // (blocks above wtop: walked, not recorded)
            if (b == wtop + 1) *jentry = j;
        } else if (colrec && lane == 0) {
            ((lds_int*)colrec)[b] = j;
        }
        bool done = j <= 0 || b == 0 || b == b_stop;
        int r = j <= 0 ? b : (b == 0 ? -1 : -2);
        if (spec && !done) {
            // merged with a segment walker: mid-segment on its recorded column, or at a segment's
            // top on its guessed column; follow merged segments to the first one that is not
            while (b < slo) slo = spec->lo(++sk);  // (b only moves down)
            int k = sk;
            int bb = b, jj = j;
            bool merged = k >= 1 && bb != spec->lo(k) && jj == uniform(((const lds_int*)spec->colrec)[bb]);
            for (;;) {
                if (merged) {
                    r = spec->res(k);
                    bb = spec->lo(k);
                    jj = spec->end(k);
                    if (r != -2) break;
                }
                merged = bb == spec->lo(k) && k + 1 < spec->K && jj == spec->gst(k + 1);
                if (!merged) break;
                ++k;
            }
            if (bb != b) {  // jumped: the walk goes on after block bb (or is over: r)
                flush(b);
                if (r != -2) {
                    res = r;
                    dump();
                    return false;
                }
                b = uniform(bb);
                j = uniform(jj);
                gtop = (b - 1) & 63;
                issue(w, b - 3, j);
                issue(wn, b - 1, j);
                issue(wa, b - 2, j);
                --b;
                return true;
            }
        }
        if (done || (b & 63) == 0) flush(b);
        src.end_block(b);
        issue(w, b - 3, j);  // unconditional (a conditional refill would merge and wait)
        if (done) {
            res = r;
            j_out = j;
            dump();
            return false;
        }
        --b;
        return true;
    };
    Win w0, w1, w2;
    issue(w0, b, j);
    issue(w1, b - 1, j);
    issue(w2, b - 2, j);
    int res = -1;
    for (;;) {
        if (!block(w0, w1, w2, res)) return res;
        if (!block(w1, w2, w0, res)) return res;
        if (!block(w2, w0, w1, res)) return res;
    }
}

template <class Src>
__device__ __forceinline__ int walk_impl(Src& src, int N, int t_start, unsigned* cmask, bool cmask_in_lds) {
    if (t_start <= 0 || N <= 0) return -1;
    int jo;
    return walk_range(src, N, (t_start - 1) >> 5, 0xFFFFFFFFu << (31 - ((t_start - 1) & 31)), 0, cmask,
                      cmask_in_lds, nullptr, nullptr, jo);
}

template <int CC>  // cells per lane of the bitmap layout (0: runtime lay.C)
__device__ int walk(const unsigned* __restrict__ bits, const Layout& lay, int N, int t_start, unsigned* cmask,
                    bool cmask_in_lds) {
    BitSrc<CC> src{bits, lay};
    return walk_impl(src, N, t_start, cmask, cmask_in_lds);
}

// Speculative walk: blocks top..0 of a walk from (t_start, N) in K segments over the workgroup's
// first K waves (SpecWalk).  Phase 1: wave 0 walks the top segment; wave k starts kSpecOverlap
// blocks above its segment from a guessed column and walks those blocks unrecorded, so that
// its path has usually merged with the true one when it enters the segment (its entry column
// is gstart[k]).  Phase 2 (after a workgroup barrier): wave 0 goes on from the top segment's
// end, jumping over whatever merged — usually every segment, with no block walked again.
// Every wave of the workgroup calls it (the barrier); returns wave 0's result (the lowest
// block, or -1), meaningful in wave 0.
constexpr int kSpecMinBlocks = 4;  // blocks per segment at least
constexpr int kSpecOverlap = 2;  // unrecorded blocks a walker starts above its segment (A/B: 1, 3, 4 slower)
// wave 0's t_start search, in walk blocks (A/B: 1, 3 or 5 within noise)
constexpr int kSpecArgmaxBlocks = 3;
// columns a walker's guess lies above the straight line, times (T - 2 N) / T (simulated on the
// decision bits, tools/walk_guess_sim.py: 0 leaves several times as many segment tops unmerged, 24 most of them)
constexpr int kSpecBias = 8;
template <class Src>
__device__ __forceinline__ int walk_spec(Src& lw, int N, int T, const float* cn, unsigned* cmask, bool cmask_in_lds,
                                         int K, int* colrec, int* sbuf, int& t_start) {
    // (one walk_range call site before the barrier and one after: every call site inlines a
    // copy of the walk, and the checkpointed walk's blocks are long)
    const int wv = uniform((int)threadIdx.x >> 6);
    const int lane = lane_id();
    SpecWalk sw;
    sw.K = K;
    sw.colrec = colrec;
    sw.gstart = sbuf;
    sw.sres = sbuf + K;
    sw.send = sbuf + 2 * K;
    int res = -1, jo = 0, tb = 0;
    unsigned fm = 0u;
    // The segments cover the blocks below T (t_start <= T): the walkers start while wave 0
    // alone finds t_start, so its segment is kSpecArgmaxBlocks shorter than theirs.  (Round 2
    // waited for a workgroup-wide t_start first: 1-2 us slower.)  K == 1: wave 0 walks alone.
    // Balanced: wave 0 takes its share less the argmax allowance, the other K - 1 segments
    // split the rest within one block of each other (a uniform length had left the last
    // walker a single block while the others walked 7 + kSpecOverlap).
    sw.top = (T - 1) >> 5;
    const int nb = sw.top + 1;
    sw.L0 = max((nb + kSpecArgmaxBlocks + K / 2) / K - kSpecArgmaxBlocks, 1);
    if (K > 1 && nb - sw.L0 < K - 1) K = max(nb - sw.L0 + 1, 1);  // (one block per walker at least)
    if (K <= 1 || sw.L0 >= nb) {
        K = 1;
        sw.L0 = nb;
        sw.Lb = 1;
        sw.ex = 0;
    } else {
        sw.Lb = (nb - sw.L0) / (K - 1);
        sw.ex = (nb - sw.L0) % (K - 1);
    }
    sw.K = K;
    sw.sres = sbuf + K;
    sw.send = sbuf + 2 * K;
    const int tref = T;
    WX_T(sp0);
    WX_TDECL(sp_am = sp0);
    // this wave's first walk: wave 0 the top segment from (t_start, N); wave k < K its segment
    // from a guessed column kSpecOverlap blocks above it
    bool go = false;
    int j0 = N, b0 = 0, stop = 0, top = 0x7fffffff, je = -1;
    unsigned fm0 = 0xFFFFFFFFu;
    int* rec = nullptr;
    if (wv == 0) {
        t_start = column_argmax<Src::kWT>(cn, T);
        WX_TSET(sp_am);
        if (t_start <= 0) {
            res = -1;  // (the reference's None)
        } else {
            tb = (t_start - 1) >> 5;
            fm = 0xFFFFFFFFu << (31 - ((t_start - 1) & 31));
            go = tb >= sw.lo(0);
            res = -3;  // (starts in a lower segment: after the barrier)
            b0 = tb;
            fm0 = fm;
            stop = sw.lo(0);
        }
    } else if (wv < K) {
        top = sw.lo(wv - 1) - 1;
        const int lo = sw.lo(wv), sb = top + kSpecOverlap;
        // guess: the straight line from (0, 0) to (tref, N), inside the cells the path can
        // occupy at time 32 (sb + 1) (column <= time, N - column <= remaining steps), moved up by
        // kSpecBias (tref - 2 N) / tref columns: a walker d columns above the true path sheds its
        // surplus on the frames that emit no token, ~d tref / (tref - N) frames, one d columns
        // below it merges only d tokens further down, ~d tref / N frames, so while N < tref / 2
        // an over-guess merges inside the overlap more often than an under-guess of the same
        // size (simulated unmerged segment tops of config 2: 16 -> 0 of 1,792)
        const int tt = 32 * (sb + 1);
        int g = (int)(((int64_t)N * tt + tref / 2 + (int64_t)kSpecBias * (tref - 2 * N)) / tref);
        g = min(max(g, max(1, N - (tref - tt))), min(N, tt));
        for (int bb = lo + lane; bb <= top; bb += kWave) colrec[bb] = -1;
        go = true;
        j0 = g;
        b0 = sb;
        stop = lo;
        rec = colrec;
    }
    if (go) {
        const int r = walk_range(lw, j0, b0, fm0, stop, cmask, cmask_in_lds, rec, nullptr, jo, top, &je);
        if (wv == 0) {
            res = r;
        } else if (lane == 0) {  // je: column entering the segment (-1: the path ended above it)
            sbuf[wv] = je;
            sbuf[K + wv] = r;
            sbuf[2 * K + wv] = jo;
        }
    }
    WX_T(sp1);
    wave_fence();
    block_fence();
    WX_T(sp2);
    // per wave (slots 6 + wave): wave 0 [argmax, first walk, barrier] cycles since entry; walkers
    // [first walk, barrier, K]
    WX_TDUMP(lane == 0 && wv <= 6, 6 + wv, wv == 0 ? sp_am - sp0 : sp1 - sp0, wv == 0 ? sp1 - sp0 : sp2 - sp0,
             wv == 0 ? sp2 - sp0 : (unsigned long long)K);
    if (wv == 0 && (res == -2 || res == -3)) {
        int j1 = N, b1 = tb;
        unsigned fm1 = fm;
        const int kl = min(lane, K - 1);  // (K <= waves <= 64)
        sw.vg = sbuf[kl];
        sw.vr = sbuf[K + kl];
        sw.ve = sbuf[2 * K + kl];
        if (res == -2) {
            // segments entered on their guessed column are the true walk's as a whole
            int k = 1;
            for (; k < K && jo == sw.gst(k); ++k) {
                res = sw.res(k);
                jo = sw.end(k);
                if (res != -2) return res;
            }
            j1 = jo;
            b1 = sw.lo(k - 1) - 1;
            fm1 = 0xFFFFFFFFu;
        }
        res = walk_range(lw, j1, b1, fm1, 0, cmask, cmask_in_lds, nullptr, &sw, jo);
    }
    return res;
}

// start[k] = k-th change frame in increasing time: a popcount prefix over the change masks
// of blocks [b_lo, b_hi] (wave 0).
__device__ void compact_starts(const unsigned* cmask, int b_lo, int b_hi, int32_t* __restrict__ start) {
    const int lane = lane_id();
    int base = 0;
    for (int b0 = b_lo; b0 <= b_hi; b0 += kWave) {
        const int b = b0 + lane;
        const unsigned m = (b <= b_hi) ? cmask[b] : 0u;
        const int c = __popc(m);
        int incl = c;  // inclusive wave scan of popcounts
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int y = __shfl_up(incl, off);
            if (lane >= off) incl += y;
        }
        int k = base + incl - c;
        unsigned mm = m;
        while (mm) {  // bit 31 = lowest frame of the block
            const int p = 31 - __clz(mm);
            start[k++] = b * kChunk + (31 - p);
            mm &= ~(1u << p);
        }
        base += __shfl(incl, kWave - 1);
    }
}

// compact_starts with every wave of the workgroup (every thread calls it): lane b of each
// 64-block group holds block b's mask and its exclusive popcount prefix; wave w stores the
// bits at positions 31 - w, 31 - w - nw, ... (token k = prefix + the set bits above the
// position: frames earlier in the block), so each wave makes 32 / nw conditional stores
// instead of wave 0 looping over every set bit of a block (1.2 us of config 2's tail).
__device__ void compact_starts_par(const unsigned* cmask, int b_lo, int b_hi, int32_t* __restrict__ start) {
    const int lane = lane_id();
    const int wv = uniform((int)threadIdx.x >> 6), nw = (int)blockDim.x >> 6;
    int base = 0;
    for (int b0 = b_lo; b0 <= b_hi; b0 += kWave) {
        const int b = b0 + lane;
        const unsigned m = (b <= b_hi) ? cmask[b] : 0u;
        const int c = __popc(m);
        int incl = c;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int y = __shfl_up(incl, off);
            if (lane >= off) incl += y;
        }
        const int k0 = base + incl - c;
        for (int p = 31 - wv; p >= 0; p -= nw) {  // bit 31 = lowest frame of the block
            const unsigned hi = p == 31 ? 0u : m >> (p + 1);
            if ((m >> p) & 1u) start[k0 + __popc(hi)] = b * kChunk + (31 - p);
        }
        base += __shfl(incl, kWave - 1);
    }
}

}  // namespace wx

#endif  // WX_DP_WALK_H
