// wx_dp_helpers.h — the helper waves of Forward (wx_dp_forward.h): they run no DP cells but stage
// the emission rows, make column 0 ahead and poll the cross-CU hand-off, barrier for barrier.
#ifndef WX_DP_HELPERS_H
#define WX_DP_HELPERS_H

#include "wx_dp_forward.h"

namespace wx {
#define WX_FWD_T template <int C, int VS, int MODE, int W, bool H, bool SP, int NH>
#define WX_FWD Forward<C, VS, MODE, W, H, SP, NH>

// Part 0's column-0 helper (wave W + 1 of a register-resident split kernel): col0_pre, the
// column-1 wave's lane-0 operand tr[t][0] + em[t, tok[0]], for the rows of every chunk, into
// column VS of the chunk's quad buffer.  tr[t][0] (alignment.py:367-370): 0 at t = 0, fp32 of
// the fp64 sum of em[0..t-1, 0] (torch CPU cumsum accumulates in double, in row order), +inf
// in the last N rows.  Barriers as helper_reg: -1, then col0_pre of chunks 0 and 1, then one
// barrier per chunk q followed by col0_pre of chunk q + 2, due before barrier q + 1.
// Pipelined so that what stands between two barriers is the fp64 chain and the 32 stores,
// not the LDS round trips around them (row reads, conversion, the write and the 16
// broadcast reads of col0_chain: ~1.3k cycles per chunk, which made this wave the last one
// at every barrier of part 0): the two columns come straight from the emission rows, loaded
// four chunks ahead (unconditional, clamped — the quad buffers and the stager are not
// involved), and chunk c + 1's doubles are converted, written to the other half of c0d and
// read back broadcast after chunk c's chain and stores, on the way to the next barrier.
// The additions and their order are col0_chain's: col0_run on the same 32 doubles.
WX_FWD_T struct WX_FWD::C0Rows {
    float e, et;  // em[t, 0], em[t, tok[0]] of row 32 c + (lane & 31)
};
WX_FWD_T __device__ void WX_FWD::col0_helper(const SegDesc& d, const float* __restrict__ E, int V, float* lds,
                                             int nch, int tok0) {
    __shared__ __attribute__((aligned(16))) double c0d[2][kChunk];
    const int T = d.T, N = d.N;
    const int l = lane_id(), rr = l & 31;
    auto load = [&](C0Rows& r, int c) {
        const float* row = E + (int64_t)min(c * kChunk + rr, T - 1) * V;
        r.e = row[0];
        r.et = row[tok0];
    };
    auto bcast = [&](int h, double(&dv)[kChunk]) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (other lanes' writes, read below)
#pragma unroll
        for (int j = 0; j < kChunk; ++j) dv[j] = c0d[h][j];
    };
    C0Rows r0, r1, r2, r3;
    load(r0, 0);
    load(r1, 1);
    load(r2, 2);
    load(r3, 3);
    double acc = 0.0;
    double dvA[kChunk], dvB[kChunk];
    WX_TDECL(acc_work = 0, acc_bar = 0);
    __syncthreads();  // barrier -1
    if (l < kChunk) c0d[0][l] = (double)r0.e;
    bcast(0, dvA);
    // chunk c: rows rc, doubles dvc; leaves chunk c + 1's doubles in dvn and reloads rc with
    // chunk c + 4
    auto iter = [&](const int c, C0Rows& rc, const C0Rows& rn, const double(&dvc)[kChunk], double(&dvn)[kChunk]) {
        WX_T(h0);
        const double a = col0_run(acc, dvc);
        acc = __builtin_bit_cast(double, readlane64(__builtin_bit_cast(unsigned long long, a), kChunk));
        float* buf = lds + (c % kBufs) * kBufFloats;
        if (l < kChunk) {
            buf[(l >> 2) * kQS + 4 * VS + (l & 3)] = col0_value(c * kChunk + l, a, T, N) + rc.et;
            c0d[(c + 1) & 1][l] = (double)rn.e;
        }
        load(rc, c + 4);
        bcast((c + 1) & 1, dvn);
        WX_T(h1);
        WX_TACC(acc_work, h1 - h0);
    };
    auto barrier = [&]() {
        WX_T(b0);
        __syncthreads();
        WX_T(b1);
        WX_TACC(acc_bar, b1 - b0);
    };
    iter(0, r0, r1, dvA, dvB);
    if (nch > 1) iter(1, r1, r2, dvB, dvA);
    for (int q = 0; q < nch;) {  // barrier q, then chunk q + 2 (rows slot (q + 2) % 4, doubles by parity)
        barrier();
        if (q + 2 < nch) iter(q + 2, r2, r3, dvA, dvB);
        if (++q >= nch) break;
        barrier();
        if (q + 2 < nch) iter(q + 2, r3, r0, dvB, dvA);
        if (++q >= nch) break;
        barrier();
        if (q + 2 < nch) iter(q + 2, r0, r1, dvA, dvB);
        if (++q >= nch) break;
        barrier();
        if (q + 2 < nch) iter(q + 2, r1, r2, dvB, dvA);
        ++q;
    }
    wait_vm();  // (no load outlives the wave)
    WX_TDUMP(l == 0, W + 1, acc_work, acc_bar, 0);  // [work, barrier wait, 0]
}

// Staging of the quad layout.  Rows are first copied row-major into a ring of kRing raw
// chunk buffers by 16-byte LDS-DMA (stage_rows: 4 instructions per chunk when V == 32,
// issued kRing - 1 chunks ahead, so each chunk has two chunk-times to land), then
// transposed LDS -> LDS into the quad buffer: lane i reads the 4 rows of its (row quad,
// column) pairs (two ds_read2_b32) and writes them as one 16-byte store.  (One-dword LDS-DMA
// straight into the quad layout needs 16 instructions per chunk: measured ~1,600 cycles of
// issue per chunk, more than a DP chunk; register staging one chunk ahead stalled on the
// loads.)  kPairs: the (row quad, column) pairs per lane.
WX_FWD_T __device__ __forceinline__ void WX_FWD::transpose_quads(const float* raw, float* buf) {
    const int l = lane_id();
    float v[kPairs][4];
#pragma unroll
    for (int m = 0; m < kPairs; ++m) {
        const int k = kWave * m + l, p = k / VS, col = k % VS;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[m][j] = raw[(4 * p + j) * VS + col];
    }
#pragma unroll
    for (int m = 0; m < kPairs; ++m) {
        const int k = kWave * m + l, p = k / VS, col = k % VS;
        *reinterpret_cast<float4*>(buf + p * kQS + 4 * col) = make_float4(v[m][0], v[m][1], v[m][2], v[m][3]);
    }
}

// The two helpers of a register-resident split kernel.  Barriers: -1, then one per chunk.
// Wave W (the stager) makes chunk q + 2's quad buffer ready before barrier q (transposed
// out of the raw ring, its DMA issued two iterations earlier); wave W + 1 (part 0 only:
// col0_helper) writes col0_pre of chunks 0 and 1 after barrier -1 and of chunk q + 2 after barrier q.
// So after barrier q the DP waves can read chunk q + 1's operands, col0_pre included,
// while they compute chunk q.  Quad buffer (q + 2) % kBufs (five) last held chunk q - 3,
// whose operand reads the DP waves waited for before chunk q - 3's steps (the column-0
// helper reads no quad buffer: it writes column VS only).
// The stager of a V == 32 batch with 16-byte aligned rows, through registers: lane l loads
// 16 bytes (columns 4 cg .. 4 cg + 3, cg = (l >> 2) & 7) of row 8 i + 4 h + j (j = l & 3,
// h = l >> 5) of a chunk with one global_load_dwordx4 per i (4 per chunk) and writes them
// into the quad layout with 16 ds_write_b32 (row quad 2 i + h, columns 4 cg + m, row j):
// no LDS-DMA ring and no LDS -> LDS transpose (which cost ~1,200 cycles per chunk and paced
// every part).  Four register sets: chunk c is loaded at iteration c - 6 (rows clamped into
// the segment, so the loads are unconditional and the compiler counts them exactly) and
// written before barrier c - 2, so each load has four chunk-times to land.
WX_FWD_T struct WX_FWD::StgSet {
    float4 v[4];
};
WX_FWD_T __device__ __forceinline__ void WX_FWD::stg_load(StgSet& s, const float* __restrict__ E, int T, int c) {
    const int l = lane_id();
    const int r = 4 * (l >> 5) + (l & 3), cg = (l >> 2) & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = min(c * kChunk + 8 * i + r, T - 1);
        s.v[i] = *reinterpret_cast<const float4*>(E + (int64_t)t * 32 + 4 * cg);
    }
}
WX_FWD_T __device__ __forceinline__ void WX_FWD::stg_write(const StgSet& s, float* buf) {
    const int l = lane_id();
    const int cg = (l >> 2) & 7;
    float* o = buf + (l >> 5) * kQS + 16 * cg + (l & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[2 * i * kQS + 0] = s.v[i].x;
        o[2 * i * kQS + 4] = s.v[i].y;
        o[2 * i * kQS + 8] = s.v[i].z;
        o[2 * i * kQS + 12] = s.v[i].w;
    }
}
WX_FWD_T __device__ void WX_FWD::stager_regs(const SegDesc& d, const float* __restrict__ E, float* lds, int nch) {
    static_assert(VS == 32, "register staging is for 32-float rows");
    const int T = d.T;
    auto buf = [&](int q) { return lds + (q % kBufs) * kBufFloats; };
    StgSet s0, s1, s2, s3;
    stg_load(s0, E, T, 0);
    stg_load(s1, E, T, 1);
    stg_load(s2, E, T, 2);
    stg_load(s3, E, T, 3);
    stg_write(s0, buf(0));
    stg_write(s1, buf(1));
    stg_load(s0, E, T, 4);
    stg_load(s1, E, T, 5);
    __syncthreads();  // barrier -1
    // iteration q: chunk q + 2 (set (q + 2) % 4) into its quad buffer, then chunk q + 6 into
    // that set; barrier q
    auto iter = [&](int q, StgSet& s) {
        if (q + 2 < nch) stg_write(s, buf(q + 2));
        stg_load(s, E, T, q + 6);
        __syncthreads();  // barrier q
    };
    int q = 0;
    for (; q + 4 <= nch; q += 4) {
        iter(q, s2);
        iter(q + 1, s3);
        iter(q + 2, s0);
        iter(q + 3, s1);
    }
    if (q < nch) iter(q++, s2);
    if (q < nch) iter(q++, s3);
    if (q < nch) iter(q++, s0);
    wait_vm();  // (no load outlives the wave)
}

// The idle helper of a part > 0 (register-resident kernels): chunk q's halo granules from
// part p - 1 into Split::xg[q & 1], re-reading until every tag matches (bounded: returns
// whether the hand-off was lost).  Only loads in this wave.  `pre` holds chunk q's first
// read, issued before barrier q - 1 (so a part that trails its predecessor finds the
// granules without a round trip inside its chunk); chunk q + 1's is issued on the way out.
WX_FWD_T __device__ bool WX_FWD::poll_halo(const Split* sp, int q, int nch, bool lost, uint64_t& pre) {
    constexpr int HL = Geo::HL;
    const int l = lane_id();
    const uint64_t* gi = sp->xin + (int64_t)q * sp->xstride + min(l, HL - 1) * C;
    uint64_t x = pre;
    bool ok = l >= HL || (unsigned)(x >> 32) == sp->tag;
    for (int it = 0; !lost && !__all(ok) && it < sp->spin; ++it) {
        x = granule_load(gi);
        ok = l >= HL || (unsigned)(x >> 32) == sp->tag;
    }
    if (l < HL) sp->xg[(q & 1) * 32 + l] = __builtin_bit_cast(float, (unsigned)x);
    pre = granule_load(gi + (int64_t)(min(q + 1, nch - 1) - q) * sp->xstride);
    return !__all(ok);
}
WX_FWD_T __device__ bool WX_FWD::helper_reg(const SegDesc& d, const float* __restrict__ E, int V, float* lds,
                                            float* raw, int nch, int tok0, bool col0, bool stage, bool x4,
                                            const Split* sp) {
    const int T = d.T;
    // the idle helper of a part > 0 that holds columns (the previous part publishes nothing
    // for a part without any)
    const bool poll = SP && !col0 && !stage && sp && sp->p > 0 &&
                      Geo::lane_of(sp->p * W, Geo::HL) < Layout::make(C, d.N, sp->lanes).G;
    bool lost = false;
    if constexpr (VS == 32) {
        if (stage && x4 && !col0) {
            stager_regs(d, E, lds, nch);
            return false;
        }
    }
    if (col0 && !stage) {  // (NH == 2: the column-0 helper does nothing else)
        col0_helper(d, E, V, lds, nch, tok0);
        return false;
    }
    auto buf = [&](int q) { return lds + (q % kBufs) * kBufFloats; };
    auto ring = [&](int q) { return raw + (q % kRing) * kChunk * VS; };
    auto rows_of = [&](int q) { return (q >= 0 && q < nch) ? min(kChunk, T - q * kChunk) : 0; };
    const ColMap cm{};  // (VS != kGatherVS: unused)
    auto issue = [&](int q) {
        if (q < nch) stage_rows<VS, 1, true>(E, V, q * kChunk, rows_of(q), ring(q), x4, cm);
    };
    // waits by DMA instruction count (stage_rows: one 16-byte instruction per 8 rows, else one
    // per row); the loads complete in order, so "at most n in flight" = everything but the
    // newest n landed
    auto instrs = [&](int q) { return q < nch ? (x4 && VS == 32 ? (rows_of(q) + 7) / 8 : rows_of(q)) : 0; };
    auto wait_all_but = [&](int q0, int q1) {  // all but chunks [q0, q1)'s DMA instructions landed
        int n = 0;
        for (int c = q0; c < q1; ++c) n += instrs(c);
        if (n >= 60) asm volatile("s_waitcnt vmcnt(60)" ::: "memory");
        else if (n >= 32) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
        else if (n >= 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
        else if (n >= 20) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
        else if (n >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else if (n >= 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    if (stage) {
        for (int q = 0; q < kRing - 1; ++q) issue(q);
        wait_all_but(2, kRing - 1);  // chunks 0 and 1 landed
        transpose_quads(ring(0), buf(0));
        if (nch > 1) transpose_quads(ring(1), buf(1));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot 0's reads done before its reuse
        issue(kRing - 1);
    }
    uint64_t pre = 0;  // poll: chunk 1's granules (first read)
    if (poll) pre = granule_load(sp->xin + (int64_t)min(1, nch - 1) * sp->xstride + min(lane_id(), Geo::HL - 1) * C);
    __syncthreads();  // barrier -1
    WX_TDECL(acc_work = 0, acc_bar = 0, acc_vm = 0);
    // one iteration: stage (chunk q + 2 transposed out of the ring — issued two iterations ago;
    // chunk q + 3's DMA may still be in flight — then chunk q + kRing issued into the slot of
    // chunk q, transposed two iterations ago), barrier q, column 0
    for (int q = 0; q < nch; ++q) {
        WX_T(h0);
        WX_TDECL(hw = h0);
        if (stage && q + 2 < nch) {
            wait_all_but(q + 3, q + kRing);  // chunk q + 2's DMA landed (later ones may be in flight)
            WX_TSET(hw);
            transpose_quads(ring(q + 2), buf(q + 2));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // its reads done: the slot is free
            issue(q + kRing);
        }
        if (poll && q > 0) {
            lost = poll_halo(sp, q, nch, lost, pre) || lost;
            WX_TSET(hw);  // (the poll counts as the DMA wait)
        }
        WX_T(h1);
        __syncthreads();  // barrier q
        WX_T(h2);
        WX_T(h3);
        WX_TACC(acc_vm, hw - h0);
        WX_TACC(acc_bar, h2 - h1);
        WX_TACC(acc_work, (h3 - h2) + (h1 - hw));
    }
    WX_TDUMP(lane_id() == 0, W + (stage ? 0 : 1), acc_work, acc_bar, acc_vm);  // [work, barrier wait, DMA wait] per helper
    return lost;
}

// The helper wave (H): mirrors the DP waves' barriers.  Before barrier q, chunks q and
// q+1 are staged and column 0 of chunk q is in c0b[q & 1].  (q0 is filled after the
// forward pass, while wave 0 walks: fill_q0.)
WX_FWD_T __device__ void WX_FWD::helper(const SegDesc& d, const float* __restrict__ E, int V, float* lds, float* c0b,
                                        int nch, bool x4, const ColMap& cm, bool col0, bool stage) {
    const int T = d.T, N = d.N;
    const int inf_from = T + 1 - N;
    double acc = 0.0;  // sum of em[0..t-1, 0], uniform
    // Rows are staged three chunks ahead (four LDS buffers) and waited for one chunk
    // ahead, so each chunk's loads have two chunk times to land: at chunk q only the
    // loads of chunk q+2 may still be in flight (vmcnt = that chunk's instruction
    // count: 4 for 16-byte staging, 32 for row staging; gathers drain fully).
    if (stage) {
        for (int i = 0; i < 3 && i < nch; ++i)
            stage_rows<VS, 1, true>(E, V, i * kChunk, min(kChunk, T - i * kChunk), lds + i * kBufFloats, x4, cm);
        wait_vm();
    }
    // chunk 0's column 0: from the staged rows, or (a column-only helper, which cannot
    // know when the other helper's staging landed) straight from the emission rows
    if (col0) {
        if (stage) {
            column0(0, T, inf_from, lds, c0b, acc);
        } else {  // chunk 0 column 0 into the 4th buffer (first staged after barrier 0)
            float* own = lds + 3 * kBufFloats;
            if (lane_id() < min(kChunk, T)) own[lane_id() * VS] = E[(int64_t)lane_id() * V];
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            column0(0, T, inf_from, own, c0b, acc);
        }
    }
    WX_TDECL(acc_c0 = 0, acc_bar = 0, acc_other = 0);
    for (int q = 0; q < nch; ++q) {
        WX_T(h0);
        // chunk q+1 must have landed; chunk q+2 (staged at q-1) may still be in flight
        if (!stage) {
        } else if (q + 2 < nch && T - (q + 2) * kChunk >= kChunk && VS != kGatherVS) {
            if (x4 && VS == 32)
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
        } else {
            wait_vm();
        }
        WX_T(h1);
        __syncthreads();
        WX_T(h2);
        if (stage && q + 3 < nch)
            stage_rows<VS, 1, true>(E, V, (q + 3) * kChunk, min(kChunk, T - (q + 3) * kChunk),
                                    lds + ((q + 3) % kBufs) * kBufFloats, x4, cm);
        WX_T(h3);
        if (col0 && q + 1 < nch)
            column0(q + 1, T, inf_from, lds + ((q + 1) % kBufs) * kBufFloats, c0b, acc);
        WX_T(h4);
        WX_TACC(acc_c0, h4 - h3);
        WX_TACC(acc_bar, h2 - h1);
        WX_TACC(acc_other, (h1 - h0) + (h3 - h2));
    }
    WX_TDUMP(lane_id() == 0, W + (stage ? 0 : 1), acc_c0, acc_bar, acc_other);
}

// Column 0 of chunk q (tr[t][0], alignment.py:367-370: 0, fp32(fp64 cumsum), +inf in
// the last N rows) into c0b[q & 1][r].  The fp64 chain runs on wave-uniform values (rows
// read as LDS broadcasts, converted ahead), one dependent v_add_f64 per row; rows past
// the segment's end feed only values nobody reads.
WX_FWD_T __device__ __forceinline__ void WX_FWD::column0(int q, int T, int inf_from, const float* buf, float* c0b,
                                                         double& acc) {
    const int t0 = q * kChunk;
    float* out = c0b + (q & 1) * kChunk;
    float e[kChunk];
#pragma unroll
    for (int r = 0; r < kChunk; ++r) e[r] = buf[r * VS];  // uniform address: broadcast
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
        out[r] = (float)acc;  // tr[t0 + r][0] before the +inf / row-0 fix-up
        acc += (double)e[r];
    }
    const int l = lane_id();
    if (l < kChunk) {
        const int t = t0 + l;
        const float v = out[l];
        out[l] = (t >= inf_from) ? INFINITY : (t == 0 ? 0.0f : v);
    }
}

#undef WX_FWD
#undef WX_FWD_T

}  // namespace wx

#endif  // WX_DP_HELPERS_H
