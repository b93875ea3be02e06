// wx_dp_forward.h — the forward pass of the alignment DP (wx_align_dp.h): Forward::run, which every
// wave of a workgroup enters, and the DP waves' chunk code.  Helper waves: wx_dp_helpers.h.
#ifndef WX_DP_FORWARD_H
#define WX_DP_FORWARD_H

#include "wx_dp_config.h"  // kChunk, Layout, Geometry, the split constants
#include "wx_dp_prims.h"
#include "wx_dp_timing.h"  // WX_T, WX_CQ, WX_TACC, WX_TDUMP
#include "wx_wave.h"

namespace wx {

// Cell values live in an ext_vector so that the one dynamic (wave-uniform) index of the
// step — the slot holding column N — lowers to s_set_gpr_idx_on/v_mov instead of scratch.
template <int C>
using cellvec = float __attribute__((ext_vector_type(C)));

// Quad-interleaved staging (the register-resident forward, Forward::kReg).  A chunk's 32 rows
// are kept as 8 row quads; quad p holds, per column c, the 4 values em[4p..4p+3, c] in 16
// contiguous bytes: float index p * QS + 4 c + (row & 3), QS = 4 (VS + 1).  One 16-byte LDS
// read then gives a lane 4 steps of its token's column (and a quarter of the lanes 4
// steps of the blank: RegOps), instead of one or two dwords per step.  Column VS of each quad is not
// staged: the column-0 helper writes the column-1 wave's lane-0 operand there (see
// Forward::col0_pre).  The stager fills it from a row-major LDS-DMA ring (Forward::transpose_quads).
template <int VS>
__host__ __device__ constexpr int quad_stride() { return 4 * (VS + 1); }
template <int VS>
__host__ __device__ constexpr int quad_buf_floats() { return 8 * quad_stride<VS>(); }

// The trellis forward pass shared by the fused and the materialising kernels.
//   MODE 0: fused — per-cell 32-step decision words -> bits, column N history -> cn.
//   MODE 1: materialise — write every trellis row (get_trellis).
//   MODE 2: checkpointed — no decision bits: at each chunk start (row 32q) every owner lane
//           stores its C cell values in the bitmap's word layout, and wave 0 the fp64
//           column-0 cumsum; the walk recomputes each block's band from them (CkSrc).  A
//           cell step is then 3 VALU (add, DPP add, maximum) instead of 5.
//
// W > 1 waves split the columns of one segment with a chunk halo instead of a per-step
// exchange: wave w >= 1 spends its first HL = ceil(32/C) lanes re-computing the last HL
// lanes of wave w-1 (>= 32 cells).  At each chunk start (row 32q) those cells are copied
// from wave w-1 through LDS; during the chunk's 32 steps the wrong value that enters at
// the halo's left edge moves right by one cell per step, so it never reaches the wave's
// own cells (cell j at row t depends only on cells j-s..j at row t-s).  The waves meet
// once per chunk at the barrier that also publishes the staged emission rows.  Halo lanes
// compute bit-identical copies (same operands, same order) and only the owning lane
// writes decisions / trellis values.
//
// H (helper): one more wave per workgroup stages the emission rows two chunks ahead and
// computes column 0 (the fp64 cumsum, +inf rows) and q0 = exp(em[t,0]) one chunk ahead, so
// the column-1 wave reads column 0 from LDS instead of running the fp64 chain per step.
// Split segments (latency mode, few segments): one segment's columns are spread over P
// workgroups ("parts", one per CU), continuing the chunk halo across CUs.  Virtual wave
// vw = part * W + wv; the first HL lanes of a part's wave 0 mirror the last HL lanes of
// the previous part's wave W-1, handed over once per 32-row chunk through global memory
// as 8-byte {value, tag} granules (one sc1 store each; the tag is the launch's 32-bit epoch and
// each chunk has its own slot, so a granule is valid on its own — no flag, no fence; the
// region is zeroed before first use and holds only granules, so a stale word carries an older
// launch's epoch and never matches).  A part lags its
// predecessor by a few chunks; the consumer prefetches each chunk's granules two chunks
// ahead.  Each part then arrives at a per-segment counter;
// the last to arrive runs the argmax, the walk and merge_repeats.
constexpr int kXSlack = 1;  // chunks a part re-builds its lag to (A/B: 1 >= 2 > 3 > 4)

struct Split {
    int p, P;         // this part, parts per segment
    int lanes;        // bitmap word stride: 64 * W * P
    unsigned tag;     // the launch epoch (32 bits, never 0)
    uint64_t* xin;    // granules from part p-1: [chunk][kHaloCells] (p > 0)
    uint64_t* xout;   // granules to part p+1 (p < P-1)
    int xstride;      // granules per chunk block of one segment boundary
    int spin;         // re-reads before a hand-off counts as lost (kMaxSpin; 0 in the recovery test)
    // Register-resident kernels: the idle helper wave of a part > 0 polls the granules of
    // chunk q and leaves their values in xg[q & 1] before barrier q; the hand-off consumer (DP
    // wave 0) reads them there after the barrier like any other wave's halo, so no DP wave
    // issues a global load.  (Routed through the consumer itself — prefetches two chunks ahead
    // by LDS-DMA, hand-counted vmcnt, its bitmap stores handed to the helper — every missed
    // prefetch cost a round trip inside the chain and the parts drifted apart: 59.7 us.)
    float* xg;  // LDS [2][32]
    float* q0l;  // LDS [T]: q0 = exp(em[t, 0]), filled by the extra walker waves (nullptr: not kept)
};

template <int C, int VS, int MODE, int W, bool H, bool SP = false, int NH = 1>
struct Forward {
    static constexpr int kRowBytes = VS * 4;
    static constexpr int kLanes = kWave * W;  // bitmap word stride (DP waves; SP: Split::lanes)
    // emission chunk buffers in LDS; kReg (declared below) keeps five: its helper restages
    // chunk q + 4 at barrier q into the buffer of chunk q - 1, the newest one no wave may still
    // be reading (the DP waves read chunk q's operands until chunk q's first step, after
    // barrier q — chunk 0's only after barrier 0)
    static constexpr int kBufs = (C == 1 && MODE == 0 && SP && NH == 2 && VS != kGatherVS) ? 5 : (H ? 4 : 2);
    // Software-pipelined LDS operands where the extra registers keep the occupancy that
    // matters: latency buckets (2 waves per SIMD by design) and one-wave buckets up to
    // C = 8; the multi-wave C = 8 buckets lose a wave per SIMD to them (A/B: -17%).
    static constexpr bool kPipelined = H || (MODE != 1 && (C <= 6 || (C == 8 && W == 1)));
    // Column 0 (tr[t][0]) read from LDS by the column-1 wave (COL kColLds): the helper wave
    // computes it (H), or — checkpointed multi-wave kernels — DP wave 1 does, a chunk ahead
    // (c0_make): the fp64 cumsum per step otherwise paced wave 0 (+25% steps in the phase timing).
    static constexpr bool kC0Lds = H || (MODE == 2 && W >= 2);
    using Geo = Geometry<C, (SP ? 2 : W)>;  // SP: always a halo (the waves span P parts)
    // Steps per unrolled group of the non-pipelined chunk (hipcc hoists the group's LDS
    // loads; a multiple of 4: column-N history is stored as float4).
    static constexpr int kU = kUnroll;
    static_assert(!(H && MODE == 1), "the materialising kernel computes column 0 in wave 0");
    // Register-resident chunks (split kernels with one cell per lane, the latency shape of
    // config 2): a chunk's operands are read into registers during the previous chunk (16-byte
    // reads of quad-interleaved rows), so the 32 steps of a chunk are a pure VALU chain — no
    // LDS read, no wait.  Micro-benchmarks (tools/ubench/step*.hip): a step costs ~20 cycles
    // of one wave alone, each LDS read issued inside the chain ~9 more.
    static constexpr bool kReg = C == 1 && MODE == 0 && SP && NH == 2 && VS != kGatherVS;
    static constexpr bool kWT = split_wt<C, VS, SP>();
    static constexpr int kBufFloats = kReg ? quad_buf_floats<VS>() : kChunk * VS;  // one chunk buffer
    static constexpr int kQS = quad_stride<VS>();

    // Per-lane state of the forward pass.
    struct State {
        cellvec<C> cur;
        unsigned w[C];
        double acc;   // W == 1 / !H: column-0 cumsum (fp64)
        float col0;   // tr[t][0] for the current step (column-1 wave)
        int t;
        // MODE 1 row stores, transposed through LDS so that every global store instruction
        // writes 256 contiguous bytes of the row: lane l stores the wave's own cells
        // jbase + l + 64 i, read from the wave's staging row at rd[i] (-1: none).
        float* rs;
        int jbase;
        int rd[C];
    };

    // SP: make xpre[] hold chunk q's halo granules (lanes < HL, C each), re-reading until
    // every tag matches.  Returns whether they were already there; bounded (sets lost).
    __device__ __forceinline__ static bool xwait(const uint64_t* xin, int xstride, int q, int l, unsigned tag,
                                                 uint64_t (&xpre)[C], bool& lost, int spin) {
        constexpr int HL = Geometry<C, 2>::HL;
        const unsigned want = tag;  // the slot already encodes the chunk; the tag is the launch
        const uint64_t* gi = xin + (int64_t)q * xstride + min(l, HL - 1) * C;  // all lanes load
        bool ok = true;
#pragma unroll
        for (int k = 0; k < C; ++k) ok = ok && (l >= HL || (unsigned)(xpre[k] >> 32) == want);
        const bool first = __all(ok);
        if (!first) {
            for (int it = 0; !lost && !__all(ok) && it < spin; ++it) {
                __builtin_amdgcn_s_sleep(2);
                ok = true;
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    xpre[k] = granule_load(gi + k);
                    ok = ok && (l >= HL || (unsigned)(xpre[k] >> 32) == want);
                }
            }
            // The re-read loop issues a data-dependent number of loads: end it with nothing in
            // flight, so that hipcc's waitcnt analysis still knows how many loads are pending
            // at the next chunk's check and waits for the two-chunk-old prefetch only (an
            // unbounded count made it wait vmcnt(0) there: the prefetch issued one chunk ago
            // and the previous chunk's bitmap stores were waited for at every chunk).
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        }
        lost = lost || !__all(ok);
        return first;
    }

    // All waves of the workgroup call run(); with H, wave W is the helper.
    __device__ __forceinline__ static bool run(const SegDesc& d, const float* __restrict__ E, int V,
                                               const int32_t* __restrict__ tok,
                                               unsigned* __restrict__ bits,  // MODE 0: segment's bitmap
                                               float* __restrict__ q0,        // MODE 0: exp(em[t,0]) per row
                                               float* __restrict__ cn,        // MODE 0: column N of rows 1..T
                                               float* __restrict__ tr,        // MODE 1: trellis
                                               float* lds /* kBufs * kBufFloats */,
                                               float* c0b /* H: 2 * kChunk column-0 values */,
                                               float* xh /* 2 * W * 64: chunk halo copies */, bool x4,
                                               const ColMap& cm /* VS == kGatherVS: column map */,
                                               float* rst = nullptr /* MODE 1: W * 64 * C row staging */,
                                               const Split* sp = nullptr /* SP */,
                                               double* c0acc = nullptr /* MODE 2: column-0 cumsum per chunk */) {
        const int wv = uniform((int)threadIdx.x >> 6);
        const int vw = SP ? sp->p * W + wv : wv;  // virtual wave (SP: across parts)
        const int lanes = SP ? sp->lanes : kLanes;
        const int T = d.T, N = d.N;
        const int nch = (T + kChunk - 1) / kChunk;
        // checkpointed multi-wave kernels: wave 1 makes column 0 of chunk q + 1 (into c0b, and
        // its cumsum at row 32 (q + 1) into c0acc) after its chunk-q steps, from em[., 0] loaded a
        // chunk ahead: the kReg helper's lane-parallel, order-preserving fp64 prefix (col0_pre)
        const bool c0prod = MODE == 2 && W >= 2 && wv == 1;
        double c0a = 0.0;  // S(32 q) of the next chunk to make (uniform)
        float c0e = 0.0f;
        const int l0 = lane_id();
        auto c0_load = [&](int qq) { return E[(int64_t)min(qq * kChunk + (l0 & 31), T - 1) * V]; };
        auto c0_make = [&](int qq, float e) {
            float x = l0 >= 32 ? e : 0.0f;
            double a = c0a;
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                a += (double)x;
                x = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x130 /* wave_shl:1 */,
                                                                       0xF, 0xF, true));
            }
            if (l0 == 0) c0acc[qq] = c0a;
            if (l0 < kChunk) c0b[(qq & 1) * kChunk + l0] = col0_value(qq * kChunk + l0, a, T, N);
            c0a = __shfl(a, kChunk);
        };
        if (c0prod && nch > 0) c0_make(0, c0_load(0));  // (before barrier 0)
        if (H && wv >= W + NH) {
            // split kernels' extra walker waves: keep the barrier count, and meanwhile fill
            // q0 = exp(em[t, 0]) (alignment.py:409's stay probabilities) into this part's LDS for
            // merge_repeats — the last part to arrive then has it at hand (fill_q0 after the walk
            // was ~1 us of config 2's tail).  64 rows per wave and chunk, loaded two chunks ahead
            // (unconditional, clamped), so no barrier waits on a load.
            float* q0l = SP ? sp->q0l : nullptr;
            const int nxw = (int)(blockDim.x >> 6) - W - NH;
            const int step = kWave * nxw;
            const int l = lane_id();
            int r0 = (wv - W - NH) * kWave;  // (uniform) first row of this wave's current group
            float e0 = 0.0f, e1 = 0.0f;
            if (q0l) {
                e0 = E[(int64_t)min(r0 + l, T - 1) * V];
                e1 = E[(int64_t)min(r0 + step + l, T - 1) * V];
            }
            if (kReg) __syncthreads();  // (barrier -1)
            for (int q = 0; q < nch; ++q) {  // 64 nxw rows per chunk of 32 rows: done by chunk nch / 2
                __syncthreads();
                if (q0l && r0 < T) {
                    if (r0 + l < T) q0l[r0 + l] = exp_cr(e0);
                    e0 = e1;
                    r0 += step;
                    e1 = E[(int64_t)min(r0 + step + l, T - 1) * V];
                }
            }
            return false;
        }
        if (H && wv >= W) {
            // NH == 2 (split kernels): wave W stages, wave W + 1 runs column 0's fp64 chain;
            // one helper doing both paced part 0 (it reached every chunk barrier last)
            const bool col0 = (!SP || sp->p == 0) && (NH == 1 || wv == W + 1);
            if constexpr (kReg) {
                int t0 = N > 0 ? tok[d.tok0] : 0;
                t0 = (t0 >= 0 && t0 < V) ? t0 : 0;
                return helper_reg(d, E, V, lds, lds + kBufs * kBufFloats, nch, t0, col0, wv == W, x4, sp);
            } else {
                helper(d, E, V, lds, c0b, nch, x4, cm, col0, NH == 1 || wv == W);
            }
            return false;
        }
        const int l = lane_id();
        const Layout L = Layout::make(C, N, lanes);
        if (MODE == 1) {
            if (threadIdx.x == 0) tr[0] = col0_value(0, 0.0, T, N);
            for (int j = (int)threadIdx.x + 1; j <= N; j += kLanes) tr[j] = -INFINITY;
        }
        if ((W > 1 || SP) && vw > 0 && Geo::lane_of(vw, Geo::HL) >= L.G) {
            // no column of this wave exists: keep the barrier count (and, without a helper,
            // this wave's share of the staging)
            if (!H && nch > 0) stage_rows<VS, W>(E, V, 0, min(kChunk, T), lds, x4, cm);
            if (kReg) __syncthreads();  // (the register-resident protocol's barrier -1)
            for (int q = 0; q < nch; ++q) {
                wait_vm();
                __syncthreads();
                if (c0prod && q + 1 < nch) c0_make(q + 1, c0_load(q + 1));
                if (!H && q + 1 < nch)
                    stage_rows<VS, W>(E, V, (q + 1) * kChunk, min(kChunk, T - (q + 1) * kChunk),
                                      lds + ((q + 1) % kBufs) * kBufFloats, x4, cm);
            }
            return false;
        }
        const int g = Geo::lane_of(vw, l);  // useful lane this lane computes
        const bool halo = vw > 0 && l < Geo::HL;
        // SP: wave W-1 hands its last HL lanes to the next part (if that part has columns);
        // wave 0 of parts > 0 takes its halo lanes from the previous part.
        const bool xpub = SP && wv == W - 1 && sp->p + 1 < sp->P && Geo::lane_of(vw + 1, Geo::HL) < L.G;
        const bool xsub = SP && wv == 0 && sp->p > 0;
        // (own_w, own_l below: column N's wave and lane)
        const int f = L.first(g), cnt = L.count(g);
        const bool is_short = g < L.n_short;
        // per-slot LDS byte offsets of em[., tok[j-1]]
        int toff[C];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int j = f + k;
            int tk = (k < cnt && j <= N) ? tok[d.tok0 + j - 1] : 0;
            tk = (tk >= 0 && tk < V) ? tk : 0;
            toff[k] = (VS == kGatherVS ? cm.rank(tk) : tk) * 4;
        }
        const int boff = (VS == kGatherVS ? cm.rank(d.blank) : d.blank) * 4;  // column 0 has rank 0
        // column N = slot C-1 of useful lane G-1
        int own_w, own_l;
        Geo::owner(L.G - 1, own_w, own_l);
        const bool owner = uniform(own_w) == vw && l == own_l;
        const bool owner_wave = uniform(own_w) == vw;
        if constexpr (kReg) {  // the register-resident split forward has its own chunk loop
            const int etq = (vw == 0 && l == 0) ? VS * 16 : toff[0] * 4;  // quad byte offset of this lane's column
            const int ebq = boff * 4 + (l & 3) * kQS * 4;                  // ... of the blank, in this lane's quad of a half-chunk
            reg_forward(sp, lds, xh, bits, cn, nch, T, wv, g, L.G, halo, xpub, xsub, owner, owner_wave, etq, ebq);
            return false;  // (a lost hand-off is the poller's to report: helper_reg)
        }

        State st;
        if (MODE == 1) {
            const int g0 = Geo::lane_of(vw, vw == 0 ? 0 : Geo::HL);  // first own useful lane
            const int g1 = min(Geo::lane_of(vw, kWave - 1), L.G - 1);
            const int jend = g1 >= g0 ? L.first(g1) + L.count(g1) - 1 : 0;
            st.jbase = g0 < L.G ? L.first(g0) : N + 1;
            const int nown = max(0, jend - st.jbase + 1);
            st.rs = rst + wv * kWave * C;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const int r = l + kWave * i;
                int gg = 0, kk = 0;
                if (r < nown) L.locate<C>(st.jbase + r - 1, gg, kk);
                st.rd[i] = r < nown ? (gg - Geo::lane_of(vw, 0)) * C + kk : -1;
            }
        }
#pragma unroll
        for (int k = 0; k < C; ++k) st.cur[k] = -INFINITY;  // row 0, columns 1..N
#pragma unroll
        for (int k = 0; k < C; ++k) st.w[k] = 0u;
        st.acc = 0.0;
        st.col0 = col0_value(0, 0.0, T, N);
        st.t = 0;
        const int inf_from = T + 1 - N;  // rows >= inf_from have column 0 = +inf

        if (!H && nch > 0) stage_rows<VS, W>(E, V, 0, min(kChunk, T), lds, x4, cm);
        // SP: halo granules prefetched two chunks ahead, odd chunks in xodd, even in xeven.
        // The chunk loop is unrolled by two for split launches so that each set stays in its
        // own registers (a loop-carried swap would make hipcc wait for both loads).
        uint64_t xodd[C], xeven[C];
        bool xlost = false;  // SP: a hand-off timed out
#pragma unroll
        for (int k = 0; k < C; ++k) xodd[k] = xeven[k] = 0;
        // Prefetches are issued by every lane, unconditionally (chunk and lane clamped into the
        // segment's granule block): a lane- or chunk-conditional load merges into the old
        // value's register, and hipcc then waits for the load right where it is issued.
        const int xl = min(l, Geo::HL - 1) * C;
        if (SP && xsub && !kReg) {
#pragma unroll
            for (int k = 0; k < C; ++k) {
                xodd[k] = granule_load(sp->xin + (int64_t)min(1, nch - 1) * sp->xstride + xl + k);
                xeven[k] = granule_load(sp->xin + (int64_t)min(2, nch - 1) * sp->xstride + xl + k);
            }
        }
        WX_TDECL(acc_steps = 0, acc_bar = 0, acc_other = 0, x_miss = 0, x_wait = 0, x_slack = 0);
        // SP: a chunk's bitmap words are stored one chunk late, after the next hand-off wait:
        // that wait drains vmcnt, and a store issued just before it would be waited for too.
        unsigned wdef[C];
#pragma unroll
        for (int k = 0; k < C; ++k) wdef[k] = 0u;
        auto store_deferred = [&](const int qd) {
#pragma unroll
            for (int k = 0; k < C; ++k) st_pub<kWT>(bits + ((int64_t)qd * C + k) * lanes + g, wdef[k]);
        };
        auto chunk_iter = [&](const int q, uint64_t(&xpre)[C]) {
            WX_T(c0);
            float* buf = lds + (q % kBufs) * kBufFloats;
            const int rows = min(kChunk, T - q * kChunk);
            float* xq = xh + (q & 1) * W * kWave;
            if (W > 1 && q > 0 && wv < W - 1 && l >= kWave - Geo::HL) {  // publish this chunk's halo
#pragma unroll
                for (int k = 0; k < C; ++k) xq[wv * kWave + (l - (kWave - Geo::HL)) * C + k] = st.cur[k];
            }
            if (SP && xpub && q > 0 && l >= kWave - Geo::HL) {  // ... and to the next part (row 32q)
                uint64_t* go = sp->xout + (int64_t)q * sp->xstride + (l - (kWave - Geo::HL)) * C;
#pragma unroll
                for (int k = 0; k < C; ++k) granule_store(go + k, st.cur[k], sp->tag);
            }
            if (SP && xpub) { WX_CQ(q, 1); }
            WX_T(c1);
            // this wave's staging (with a helper, DP waves stage nothing).  Single-CU fused
            // launches: not the previous chunk's C bitmap stores, issued last (the wait would
            // expose a store round trip per chunk)
            if (!H) wait_vm();
            __syncthreads();
            WX_T(c2);
            if (wv == 0) { WX_CQ(q, 0); }
            if (W > 1 && q > 0 && halo && wv > 0) {
#pragma unroll
                for (int k = 0; k < C; ++k) st.cur[k] = xq[(wv - 1) * kWave + l * C + k];
            }
            if (SP && xsub && q > 0) {
                // Halo of row 32q from the previous part: the granules prefetched two chunks
                // ago (the sc1 load takes longer than a chunk).  A part must trail its
                // predecessor by more than the prefetch distance plus the hand-off latency for
                // the prefetch to find them; at chunk 1, and after any miss, it therefore also
                // waits until chunk q + kXSlack is visible (re-building that slack once instead
                // of paying a round trip every chunk).  Waits are bounded: a lost hand-off
                // marks the segment failed.  (An LDS-DMA landing ring with hand-counted vmcnt
                // measured no better.)
                WX_T(x0);
                const bool missed = !xwait(sp->xin, sp->xstride, q, l, sp->tag, xpre, xlost, sp->spin);
                WX_CQ(q, 2);
                if (l < Geo::HL) {
#pragma unroll
                    for (int k = 0; k < C; ++k) st.cur[k] = __builtin_bit_cast(float, (unsigned)xpre[k]);
                }
                WX_T(x1);
                if ((missed || q == 1) && q + kXSlack < nch) {
                    uint64_t tmp[C];
#pragma unroll
                    for (int k = 0; k < C; ++k) tmp[k] = 0;
                    xwait(sp->xin, sp->xstride, q + kXSlack, l, sp->tag, tmp, xlost, sp->spin);
                }
                WX_T(x2);
                WX_TACC(x_miss, missed ? 1 : 0);
                WX_TACC(x_wait, x1 - x0);
                WX_TACC(x_slack, x2 - x1);
                // this set's next chunk, q + 2 (the old values are dead: keep the load below)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < C; ++k)
                    xpre[k] = granule_load(sp->xin + (int64_t)min(q + 2, nch - 1) * sp->xstride + xl + k);
            }
            if (SP && MODE == 0 && q > 0 && !halo && g < L.G) store_deferred(q - 1);
            if constexpr (MODE == 2) {
                // checkpoint row 32q (before the chunk's steps; after the barrier, so that the
                // next chunk's vmcnt wait finds these stores a chunk old): the owner lanes' cells
                // in the bitmap word layout, and the fp64 cumsum behind column 0 (wave 0: every
                // lane holds it, alignment.py:368)
                if (!halo && g < L.G) {
                    float* ck = reinterpret_cast<float*>(bits);
#pragma unroll
                    for (int k = 0; k < C; ++k) ck[((int64_t)q * C + k) * lanes + g] = st.cur[k];
                }
                if (!kC0Lds && vw == 0 && l == 0) c0acc[q] = st.acc;
            }
            if (c0prod && q + 1 < nch) c0e = c0_load(q + 1);  // (consumed after this chunk's steps)
            if (!H) {
                if (q + 1 < nch)
                    stage_rows<VS, W>(E, V, (q + 1) * kChunk, min(kChunk, T - (q + 1) * kChunk),
                                      lds + ((q + 1) % kBufs) * kBufFloats, x4, cm);
                if (MODE != 1 && wv == 0 && l < rows) q0[q * kChunk + l] = exp_cr(buf[l * VS]);  // never idle
            }
            const char* bb = reinterpret_cast<const char*>(buf);
            const float* c0q = kC0Lds ? c0b + (q & 1) * kChunk : nullptr;
            WX_T(c3);
            if (vw == 0) {
                chunk<true>(bb, c0q, rows, toff, boff, st, inf_from, is_short, halo, f, cnt, owner, N, cn, tr);
            } else {
                chunk<false>(bb, c0q, rows, toff, boff, st, inf_from, is_short, halo, f, cnt, owner, N, cn, tr);
            }
            if (c0prod && q + 1 < nch) c0_make(q + 1, c0e);  // (read after barrier q + 1)
            WX_T(c4);
            WX_TACC(acc_steps, c4 - c3);
            WX_TACC(acc_bar, c2 - c1);
            WX_TACC(acc_other, (c1 - c0) + (c3 - c2));
            if (MODE == 0) {
                const int sh = kChunk - rows;  // keep bit 31 = first step of the block
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const unsigned wq = (sh == 0) ? st.w[k] : (st.w[k] << sh);
                    if (SP)
                        wdef[k] = wq;
                    else if (!halo && g < L.G)  // (lanes past column N: words the walk never reads)
                        bits[((int64_t)q * C + k) * lanes + g] = wq;
                    st.w[k] = 0u;
                }
            }
        };
        if constexpr (SP) {
            for (int q = 0; q < nch; q += 2) {
                chunk_iter(q, xeven);
                if (q + 1 < nch) chunk_iter(q + 1, xodd);
            }
            if (MODE == 0 && nch > 0 && !halo && g < L.G) store_deferred(nch - 1);
        } else {
            for (int q = 0; q < nch; ++q) chunk_iter(q, xeven);
        }
        WX_TDUMP(l == 0 && MODE != 1, wv, acc_steps, acc_bar, acc_other,
                 if (SP && xsub) { WX_TSTORE(14, x_miss, x_wait, x_slack) });
        return xlost;
    }

    // ---------------------------------------------------------------- register-resident chunks
    // The blank operand is the same 32 numbers in every lane of a wave, so a lane keeps only a
    // quarter of them: in half-chunk h (16 steps) lane l holds blank quad 4 h + (l & 3), i.e.
    // em[16 h + 4 (l & 3) .. + 3, blank], and a step takes its blank from the lane of its own
    // quad of four lanes that holds it (reg_steps4) — 8 VGPRs per operand set instead of 32, and
    // one 16-byte LDS read per 16 steps (four addresses per wave) instead of one per 4.
    struct RegOps {
        float4 et[kChunk / 4];   // em[t, tok] of this lane's cell (column-1 wave, lane 0: col0_pre's value)
        float4 eb[kChunk / 16];  // em[t, blank]: blank quad 4 h + (lane & 3) of half-chunk h
    };
    // ebq: the blank's quad byte offset plus this lane's (l & 3) quads (run()).
    __device__ __forceinline__ static void reg_load(RegOps& o, const char* buf, int etq, int ebq) {
#pragma unroll
        for (int p = 0; p < kChunk / 4; ++p) {
            o.et[p] = *reinterpret_cast<const float4*>(buf + p * kQS * 4 + etq);
            if (p % 4 == 0) o.eb[p / 4] = *reinterpret_cast<const float4*>(buf + p * kQS * 4 + ebq);
        }
    }
    // Four time steps of one cell (alignment.py:372-378), hand-ordered so that the chain
    // through the cell value (maximum -> next step's DPP add) needs no wait states: the DPP's
    // source is read two instructions after the maximum that wrote it (the addc and the stay
    // add sit in between).  One asm block per four steps: hipcc cannot see inside a block and
    // pads an s_nop at every block boundary whose next block might read a fresh VGPR through
    // DPP.  Lane 0's left input is zero-filled: in the column-1 wave its operand `et` is
    // col0_pre's tr[t][0] + em[t, tok[0]] (0 + x is x for every x the DP can tell apart: it
    // only compares values and takes maxima), elsewhere a halo lane's don't-care.  n[k] =
    // the cell value after step k.
    // The stay add takes the blank of step 4 p + k from component k of `eb` as held by lane
    // R = p % 4 of the lane's quad (quad_perm:[R,R,R,R]; eb + cur is cur + eb bit for bit).  Its
    // DPP source is an operand register: written by a ds_read (reg_load, reg_chunk) and by
    // no VALU instruction, so the VALU-write -> DPP-read wait states concern `cur` alone, which
    // the stay add reads as its plain second source.  quad_perm reads other lanes' registers, which
    // delivers the value only from active lanes: EXEC is full wherever a DP wave runs these blocks
    // (every branch of reg_forward around reg_chunk is wave-uniform; its lane-conditional
    // stores end before the chunk's first block).  Both were checked in the gfx950 code of
    // <1, 32, 3> and <1, 32, 4>: every quad_perm source is last written by a ds_read_b128, and
    // no EXEC write or branch stands inside a chunk.
#define WX_REG_STEP(CUR, NC, ET, EB, R)                                                               \
    "v_add_f32_dpp %[s], %[" #EB "], %[" #CUR "] quad_perm:[" #R "," #R "," #R "," #R "] row_mask:0xf bank_mask:0xf\n\t" \
    "v_add_f32_dpp %[c], %[" #CUR "], %[" #ET "] wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
    "v_cmp_gt_f32 vcc, %[c], %[s]\n\t"                                                              \
    "v_maximum3_f32 %[" #NC "], %[s], %[c], %[c]\n\t"                                               \
    "v_addc_co_u32 %[w], vcc, %[w], %[w], vcc\n\t"
#define WX_REG_STEPS4(R)                                                                            \
    WX_REG_STEP(cur, n0, e0, b0, R) WX_REG_STEP(n0, n1, e1, b1, R) WX_REG_STEP(n1, n2, e2, b2, R)   \
        WX_REG_STEP(n2, n3, e3, b3, R)
#define WX_REG_OPERANDS                                                                                 \
    : [n0] "=&v"(n[0]), [n1] "=&v"(n[1]), [n2] "=&v"(n[2]), [n3] "=&v"(n[3]), [w] "+v"(w), [s] "=&v"(s),  \
      [c] "=&v"(c)                                                                                          \
    : [cur] "v"(cur), [e0] "v"(et.x), [e1] "v"(et.y), [e2] "v"(et.z), [e3] "v"(et.w), [b0] "v"(eb.x),     \
      [b1] "v"(eb.y), [b2] "v"(eb.z), [b3] "v"(eb.w)                                                         \
    : "vcc"
    // FIRST: `cur` may have just been written by a VALU op (halo copy-in); R: the quad lane
    // holding these four steps' blank
    template <bool FIRST, int R>
    __device__ __forceinline__ static void reg_steps4(float cur, unsigned& w, const float4& et, const float4& eb,
                                                      float (&n)[4]) {
        static_assert(0 <= R && R < 4, "quad lane");
        float s, c;
        if constexpr (FIRST)
            asm volatile("s_nop 1\n\t" WX_REG_STEPS4(0) WX_REG_OPERANDS);
        else if constexpr (R == 0)
            asm volatile(WX_REG_STEPS4(0) WX_REG_OPERANDS);
        else if constexpr (R == 1)
            asm volatile(WX_REG_STEPS4(1) WX_REG_OPERANDS);
        else if constexpr (R == 2)
            asm volatile(WX_REG_STEPS4(2) WX_REG_OPERANDS);
        else
            asm volatile(WX_REG_STEPS4(3) WX_REG_OPERANDS);
        static_assert(!FIRST || R == 0, "the chunk's first block takes quad lane 0's blank");
    }
#undef WX_REG_OPERANDS
#undef WX_REG_STEPS4
#undef WX_REG_STEP
    // 32 steps on operands `o`, issuing the next chunk's operand reads (n, from buffer nb) one
    // quad ahead of each group of four steps (the blank's: one per half-chunk).  OWN: this wave
    // holds column N (the others have no column-N code); hist: the cell value after each step,
    // which reg_forward stores.
    template <bool OWN, int P>
    __device__ __forceinline__ static void reg_group(const RegOps& o, RegOps& n, const char* nb, int etq, int ebq,
                                                     float& cur, unsigned& w, float (&hist)[OWN ? kChunk : 1]) {
        n.et[P] = *reinterpret_cast<const float4*>(nb + P * kQS * 4 + etq);
        if constexpr (P % 4 == 0) n.eb[P / 4] = *reinterpret_cast<const float4*>(nb + P * kQS * 4 + ebq);
        __builtin_amdgcn_sched_barrier(0);
        float nv[4];
        reg_steps4<P == 0, P % 4>(cur, w, o.et[P], o.eb[P / 4], nv);
        if constexpr (OWN) {
#pragma unroll
            for (int j = 0; j < 4; ++j) hist[4 * P + j] = nv[j];
        }
        cur = nv[3];
        __builtin_amdgcn_sched_barrier(0);
    }
    template <bool OWN>
    __device__ __forceinline__ static void reg_chunk(const RegOps& o, RegOps& n, const char* nb, int etq, int ebq,
                                                     float& cur, unsigned& w, float (&hist)[OWN ? kChunk : 1]) {
        static_assert(kChunk == 32, "eight groups of four steps");
        reg_group<OWN, 0>(o, n, nb, etq, ebq, cur, w, hist);
        reg_group<OWN, 1>(o, n, nb, etq, ebq, cur, w, hist);
        reg_group<OWN, 2>(o, n, nb, etq, ebq, cur, w, hist);
        reg_group<OWN, 3>(o, n, nb, etq, ebq, cur, w, hist);
        reg_group<OWN, 4>(o, n, nb, etq, ebq, cur, w, hist);
        reg_group<OWN, 5>(o, n, nb, etq, ebq, cur, w, hist);
        reg_group<OWN, 6>(o, n, nb, etq, ebq, cur, w, hist);
        reg_group<OWN, 7>(o, n, nb, etq, ebq, cur, w, hist);
    }

    // The DP waves' chunk loop of the register-resident split forward (run() sends them here;
    // C = 1, so a lane is one cell and HL = 32 halo lanes).  Per chunk q: barrier q; the halo of
    // row 32 q comes in; chunk q - 1's decision word goes out (one chunk late, as in run());
    // the 32 steps (reg_chunk), which also read chunk q + 1's operands; then row 32 (q + 1) is
    // published for barrier q + 1 — to the next wave through xh, to the next part as granules —
    // and the owner lane stores the chunk's column-N history.
    // Barriers: every DP wave that comes here executes barrier -1 and then exactly one barrier per
    // chunk, nch in all (iter() has the only __syncthreads of the loop and is called once for
    // every q in [0, nch)), which is what run()'s other routes — helpers, extra walker waves,
    // waves without a column — execute.  Nothing here waits, polls or sleeps.
    // What sits between two chunks' steps is kept short (it is paid 47 times by every wave of
    // config 2, on the chain through the parts):
    //   * chunk 0 and the two parities are separate copies (FIRST, PAR), the ring slot is a
    //     running byte offset, pointers advance by their strides: nothing is derived from q;
    //   * the two LDS accesses have no branch and no wave condition: every lane writes (the
    //     lanes that publish nothing into a pad slot of their wave's xh row, slots 32..63 of
    //     each 64: a C = 1 halo fills only 0..31), and every wave reads through one pointer pair
    //     set up here — the previous wave's row, the poller's Split::xg or, in the column-1 wave,
    //     its own row — and keeps the value in its halo lanes only (a select; hipcc makes it one
    //     ds_read under the halo lanes' mask);
    //   * the publish is issued directly behind the last step, so its LDS latency runs under
    //     the rest of the boundary;
    //   * a partial last chunk runs all 32 steps on stale rows (harmless: nothing reads the
    //     cell state after the last chunk, and column N's rows past T land in the padding);
    //     the bits of its steps past T are dropped from its word once, after the loop.
    __device__ __forceinline__ static void reg_forward(const Split* sp, float* lds, float* xh,
                                                       unsigned* __restrict__ bits, float* __restrict__ cn, int nch,
                                                       int T, int wv, int g, int G, bool halo, bool xpub,
                                                       bool xsub, bool owner, bool owner_wave, int etq, int ebq) {
        constexpr int HL = Geo::HL;
        static_assert(C == 1 && 2 * HL == kWave, "pad slots: a C = 1 halo fills half of a wave's xh row");
        const int l = lane_id();
        const int lanes = sp->lanes;
        constexpr int kBufBytes = kBufFloats * 4;
        // LDS: where this lane publishes (chunk parity 0; parity 1 is W * kWave floats on) ...
        float* const hw = xh + wv * kWave + (l ^ HL);  // lanes >= 32: slots 0..31; the others: pad
        // ... and where its halo value of an even / odd chunk arrives: the previous wave's row,
        // or (wave 0 of a part > 0) the poller's Split::xg; the column-1 wave reads its own row
        const float* hr[2];
        hr[0] = (wv > 0 ? xh + (wv - 1) * kWave : (xsub ? sp->xg : xh)) + (l & (HL - 1));
        hr[1] = hr[0] + ((wv > 0 || !xsub) ? W * kWave : 32);
        const bool own_word = !halo && g < G;                         // lanes whose decision word is kept
        unsigned* wp = bits + ((int64_t)g - lanes);                   // chunk q - 1's word
        uint64_t* gp = sp->xout + (l - (kWave - HL));                 // chunk q's granule (lanes >= 32)
        int t0 = 0;                                                   // column N: rows t0 + 1 .. t0 + 32
        int rn = kBufBytes;                                           // ring byte offset of chunk q + 1
        float cur = -INFINITY;                                        // row 0, columns 1..N
        unsigned w = 0u, wdef = 0u;                                   // this chunk's word, the last one's
        RegOps opsA, opsB;  // the operands of the chunk being computed and of the next one, swapped per chunk
        WX_TDECL(acc_steps = 0, acc_bar = 0, acc_other = 0);
        __syncthreads();  // barrier -1 (helper_reg: the column-0 helper's first two chunks)
        // OWN (compile time): the wave holding column N (the only one with column-N stores; the
        // others have no branch around them: a taken branch per eight steps cost the DP waves
        // ~20% of their step time).
        auto iter = [&](const int q, auto first, auto par, RegOps& o, RegOps& n, auto own) {
            constexpr bool FIRST = decltype(first)::value, OWN = decltype(own)::value;
            constexpr int PAR = decltype(par)::value ? 1 : 0;
            WX_T(c1);
            __syncthreads();  // barrier q
            WX_T(c2);
            if (wv == 0) { WX_CQ(q, 0); }
            if constexpr (FIRST) {
                reg_load(o, reinterpret_cast<const char*>(lds), etq, ebq);
            } else {
                const float hv = *hr[PAR];
                cur = halo ? hv : cur;
                if (own_word) st_pub<kWT>(wp, wdef);
            }
            wp += lanes;
            const char* nb = reinterpret_cast<const char*>(lds) + rn;
            rn = rn + kBufBytes == kBufs * kBufBytes ? 0 : rn + kBufBytes;
            WX_T(c3);
            float hist[OWN ? kChunk : 1];
            reg_chunk<OWN>(o, n, nb, etq, ebq, cur, w, hist);
            WX_T(c4);
            hw[(PAR ^ 1) * W * kWave] = cur;  // (every lane writes; after the last chunk: read by no one)
            gp += sp->xstride;
            if (xpub && q + 1 < nch) {
                if (l >= kWave - HL) granule_store(gp, cur, sp->tag);
                WX_CQ(q + 1, 1);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (OWN && owner) {
                // rows t0 + 1 .. t0 + 32 -> cn[t0 .. t0 + 31], once per chunk and whole: rows past T
                // land in the segment's padding (kCnPad).  (Stored per 8 steps inside the chain,
                // with a partial-group path, they cost the pacing wave a taken branch and an EXEC
                // round trip per 8 steps: 59.7 -> 55.3 -> ... us.)
                // Eight 16-byte stores, written through (sc1, kWT): the last part reads them with
                // sc1 loads and the arrival needs no release (32 single 4-byte sc1 stores had cost
                // more than the release).
#pragma unroll
                for (int i = 0; i < kChunk / 4; ++i)
                    st_pub4<kWT>(cn, t0 + 4 * i, make_float4(hist[4 * i], hist[4 * i + 1], hist[4 * i + 2], hist[4 * i + 3]));
            }
            t0 += kChunk;
            wdef = w;
            w = 0u;
            WX_T(c5);
            WX_TACC(acc_steps, c4 - c3);
            WX_TACC(acc_bar, c2 - c1);
            WX_TACC(acc_other, (c3 - c2) + (c5 - c4));
        };
        auto loop = [&](auto own) {
            if (nch > 0) iter(0, BoolTag<true>{}, BoolTag<false>{}, opsA, opsB, own);
            for (int q = 1; q < nch; q += 2) {
                iter(q, BoolTag<false>{}, BoolTag<true>{}, opsB, opsA, own);
                if (q + 1 < nch) iter(q + 1, BoolTag<false>{}, BoolTag<false>{}, opsA, opsB, own);
            }
        };
        if (owner_wave)
            loop(BoolTag<true>{});
        else
            loop(BoolTag<false>{});
        // the last chunk's word: bit 31 is its first step, the bits of the steps past T are dropped
        if (nch > 0 && own_word) st_pub<kWT>(wp, wdef & (0xFFFFFFFFu << (nch * kChunk - T)));
        WX_TDUMP(l == 0, wv, acc_steps, acc_bar, acc_other, if (xsub) { WX_TSTORE(14, 0, 0, 0) });
    }

    // Helper waves: the waves beyond the W DP waves (run() sends them here; they keep its barrier count): helper (H),
    // helper_reg (kReg) and their parts.  Defined in wx_dp_helpers.h, which whoever instantiates run() includes.
    __device__ static void helper(const SegDesc& d, const float* __restrict__ E, int V, float* lds, float* c0b,
                                  int nch, bool x4, const ColMap& cm, bool col0, bool stage = true);
    __device__ __forceinline__ static void column0(int q, int T, int inf_from, const float* buf, float* c0b,
                                                   double& acc);
    __device__ static bool helper_reg(const SegDesc& d, const float* __restrict__ E, int V, float* lds, float* raw,
                                      int nch, int tok0, bool col0, bool stage, bool x4, const Split* sp = nullptr);
    struct C0Rows;
    __device__ static void col0_helper(const SegDesc& d, const float* __restrict__ E, int V, float* lds, int nch,
                                       int tok0);
    static constexpr int kRing = 4;  // (A/B: 8 was 1.5 us slower on config 2)
    static constexpr int kPairs = 8 * VS / kWave;  // (row quad, column) pairs per lane
    __device__ __forceinline__ static void transpose_quads(const float* raw, float* buf);
    struct StgSet;
    __device__ __forceinline__ static void stg_load(StgSet& s, const float* __restrict__ E, int T, int c);
    __device__ __forceinline__ static void stg_write(const StgSet& s, float* buf);
    __device__ static void stager_regs(const SegDesc& d, const float* __restrict__ E, float* lds, int nch);
    __device__ static bool poll_halo(const Split* sp, int q, int nch, bool lost, uint64_t& pre);

    // One chunk's steps: unrolled groups of kUnroll with immediate LDS row offsets, then the
    // remainder.  WAVE0: this wave holds column 1 (its left input is column 0).
    template <bool WAVE0>
    __device__ __forceinline__ static void chunk(const char* bb, const float* c0q, int rows, const int (&toff)[C],
                                                 int boff, State& st, int inf_from, bool is_short, bool halo, int f,
                                                 int cnt, bool owner, int N, float* __restrict__ cn,
                                                 float* __restrict__ tr) {
        constexpr int kColLds = 3, kColFinite = 1, kColAny = 2;
        if (kPipelined && rows == kChunk) {  // software-pipelined full chunk
            if (!WAVE0)
                pipelined_chunk<0>(bb, c0q, toff, boff, st, inf_from, false, halo, f, cnt, owner, N, cn, tr);
            else if (kC0Lds)
                pipelined_chunk<kColLds>(bb, c0q, toff, boff, st, inf_from, is_short, halo, f, cnt, owner, N, cn, tr);
            else if (st.t + kChunk < inf_from)
                pipelined_chunk<kColFinite>(bb, c0q, toff, boff, st, inf_from, is_short, halo, f, cnt, owner, N, cn, tr);
            else
                pipelined_chunk<kColAny>(bb, c0q, toff, boff, st, inf_from, is_short, halo, f, cnt, owner, N, cn, tr);
            return;
        }
        int r = 0;
        for (; r + kU <= rows; r += kU) {
            const char* gb = bb + r * kRowBytes;
            const char* ga[C];
#pragma unroll
            for (int k = 0; k < C; ++k) ga[k] = gb + toff[k];
            float hist[kU];  // column N after each step (owner lane)
            if (!WAVE0 || kC0Lds || st.t + kU < inf_from) {  // column 0 from LDS, or finite for the group
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    step<!WAVE0 ? 0 : (kC0Lds ? kColLds : kColFinite)>(gb, ga, u * kRowBytes, boff, c0q + r + u, st,
                                                                 inf_from, is_short, halo, f, cnt, N, tr);
                    hist[u] = st.cur[C - 1];
                    ++st.t;
                }
            } else {
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    step<kColAny>(gb, ga, u * kRowBytes, boff, c0q, st, inf_from, is_short, halo, f, cnt, N, tr);
                    hist[u] = st.cur[C - 1];
                    ++st.t;
                }
            }
            if (MODE != 1 && owner) {  // rows t-kU+1 .. t at cn[t-kU .. t-1] (16-byte aligned)
#pragma unroll
                for (int i = 0; i < kU / 4; ++i)
                    st_pub4<kWT>(cn, st.t - kU + 4 * i, make_float4(hist[4 * i], hist[4 * i + 1], hist[4 * i + 2], hist[4 * i + 3]));
            }
        }
        for (; r < rows; ++r) {
            const char* gb = bb + r * kRowBytes;
            const char* ga[C];
#pragma unroll
            for (int k = 0; k < C; ++k) ga[k] = gb + toff[k];
            step<!WAVE0 ? 0 : (kC0Lds ? kColLds : kColAny)>(gb, ga, 0, boff, c0q + r, st, inf_from, is_short, halo, f,
                                                       cnt, N, tr);
            if (MODE != 1 && owner) st_pub<kWT>(cn + st.t, st.cur[C - 1]);
            ++st.t;
        }
    }

    // A full 32-step chunk with the LDS operands of step u+2 and u+3 loaded while step u
    // computes.  sched_barrier keeps the scheduler from sinking the loads back to their uses
    // (it does, to minimise registers); the waitcnt pass counts them exactly, since LDS
    // returns in order.
    template <int COL>
    __device__ __forceinline__ static void pipelined_chunk(const char* bb, const float* c0q, const int (&toff)[C],
                                                           int boff, State& st, int inf_from, bool is_short,
                                                           bool halo, int f, int cnt, bool owner, int N,
                                                           float* __restrict__ cn, float* __restrict__ tr) {
        const char* ga[C];
#pragma unroll
        for (int k = 0; k < C; ++k) ga[k] = bb + toff[k];
        Row rw[kChunk];
        // COL 3 (column 0 from the helper's LDS row): the chunk's 32 values in 8 16-byte
        // loads up front instead of an address move + ds_read_b32 per step in the wave that
        // paces the chain (the column-1 wave)
        float c0r[COL == 3 ? kChunk : 1];
        if constexpr (COL == 3) {
#pragma unroll
            for (int i = 0; i < kChunk / 4; ++i) {
                const float4 v = reinterpret_cast<const float4*>(c0q)[i];
                c0r[4 * i] = v.x;
                c0r[4 * i + 1] = v.y;
                c0r[4 * i + 2] = v.z;
                c0r[4 * i + 3] = v.w;
            }
        }
        constexpr int LC = COL == 3 ? 4 : COL;  // load_row without the per-step column-0 read
        auto c0_of = [&](Row& r, int u) {
            if constexpr (COL == 3) r.c0 = c0r[u];
        };
        load_row<LC>(bb, ga, 0, boff, c0q, rw[0]);
        load_row<LC>(bb, ga, kRowBytes, boff, c0q + 1, rw[1]);
        c0_of(rw[0], 0);
        c0_of(rw[1], 1);
        float hist[kUnroll];
#pragma unroll
        for (int u = 0; u < kChunk; ++u) {
            if ((u & 1) == 0 && u + 2 < kChunk) {
                load_row<LC>(bb, ga, (u + 2) * kRowBytes, boff, c0q + u + 2, rw[u + 2]);
                load_row<LC>(bb, ga, (u + 3) * kRowBytes, boff, c0q + u + 3, rw[u + 3]);
                c0_of(rw[u + 2], u + 2);
                c0_of(rw[u + 3], u + 3);
            }
            __builtin_amdgcn_sched_barrier(0);
            advance<COL>(bb, u * kRowBytes, c0q + u, rw[u], st, inf_from, is_short, halo, f, cnt, N, tr);
            hist[u & (kUnroll - 1)] = st.cur[C - 1];
            ++st.t;
            if (MODE != 1 && (u & (kUnroll - 1)) == kUnroll - 1 && owner) {
                st_pub4<kWT>(cn, st.t - kUnroll, make_float4(hist[0], hist[1], hist[2], hist[3]));
                st_pub4<kWT>(cn, st.t - kUnroll + 4, make_float4(hist[4], hist[5], hist[6], hist[7]));
            }
        }
    }

    // One time step t -> t+1 (alignment.py:372-378).  COL: 0 = not the column-1 wave (lane
    // 0's left input is a halo edge, don't-care); column-1 wave: 1 = column 0 finite for the
    // next row, 2 = general column 0, 3 = column 0 read from the helper's LDS row.
    template <int COL>
    __device__ __forceinline__ static void step(const char* gb, const char* (&ga)[C], int ro, int boff,
                                                const float* c0, State& st, int inf_from, bool is_short, bool halo,
                                                int f, int cnt, int N, float* __restrict__ tr) {
        Row rw;
        load_row<COL>(gb, ga, ro, boff, c0, rw);
        advance<COL>(gb, ro, c0, rw, st, inf_from, is_short, halo, f, cnt, N, tr);
    }

    // The LDS operands of one step: em[t, blank], em[t, tok[j-1]] per slot, column 0 (COL 3).
    struct Row {
        float eb;
        float et[C];
        float c0;
    };
    template <int COL>
    __device__ __forceinline__ static void load_row(const char* gb, const char* (&ga)[C], int ro, int boff,
                                                    const float* c0, Row& rw) {
        rw.eb = *reinterpret_cast<const float*>(gb + ro + boff);
#pragma unroll
        for (int k = 0; k < C; ++k) rw.et[k] = *reinterpret_cast<const float*>(ga[k] + ro);
        if (COL == 3) rw.c0 = *c0;
        if (COL == 1 || COL == 2) rw.c0 = *reinterpret_cast<const float*>(gb + ro);  // em[t, 0]
    }

    template <int COL>
    __device__ __forceinline__ static void advance(const char* gb, int ro, const float* c0, const Row& rw, State& st,
                                                   int inf_from, bool is_short, bool halo, int f, int cnt, int N,
                                                   float* __restrict__ tr) {
        const float eb = rw.eb;
        const float(&et)[C] = rw.et;
        // last cell of the lane to the left (short lanes end at slot C-2)
        const float src = (C > 1 && is_short) ? st.cur[C > 1 ? C - 2 : 0] : st.cur[C - 1];
        // Lane 0's left input is column 0 in the column-1 wave and a halo lane's don't-care
        // elsewhere: there the DPP zero-fills (bound_ctrl).  In the column-1 wave lane 63
        // passes column 0 round to lane 0 instead (wave_ror:1; lane 63's own last cell feeds
        // no lane of this wave).  Either way every lane's source is a plain register, so
        // hipcc fuses the shift into the add (v_add_f32_dpp) and no v_mov sets up `old`.
        float left;
        if (COL) {
            const float c0v = COL == 3 ? rw.c0 : st.col0;
            const float src2 = lane_id() == kWave - 1 ? c0v : src;
            left = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, src2), 0x13C /* wave_ror:1 */,
                                                                      0xF, 0xF, true));  // (no lane is out of range)
        } else {
            left = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, src), 0x138 /* wave_shr:1 */,
                                                                      0xF, 0xF, true));
        }
#pragma unroll
        for (int k = C - 1; k >= 0; --k) {
            const float s = st.cur[k] + eb;
            const float c = (k == 0 ? left : st.cur[k > 0 ? k - 1 : 0]) + et[k];
            if (MODE == 0) st.w[k] = shift_in(st.w[k], c, s);
            st.cur[k] = nan_max(s, c);
        }
        if (COL == 1 || COL == 2) {
            const float e0 = rw.c0;
            st.acc += (double)e0;
            st.col0 = (COL == 1 || st.t + 1 < inf_from) ? (float)st.acc : INFINITY;
        }
        if (MODE == 1) {
            float* row = tr + (int64_t)(st.t + 1) * ((int64_t)N + 1);
            if (COL && lane_id() == 0)
                row[0] = COL == 3 ? (st.t + 1 < inf_from ? c0[1] : INFINITY) : st.col0;
            float* rw = st.rs + lane_id() * C;  // every lane stages its C slots (in-order LDS)
            if constexpr (C % 4 == 0) {
#pragma unroll
                for (int k = 0; k < C; k += 4)
                    *reinterpret_cast<float4*>(rw + k) = make_float4(st.cur[k], st.cur[k + 1], st.cur[k + 2], st.cur[k + 3]);
            } else if constexpr (C % 2 == 0) {
#pragma unroll
                for (int k = 0; k < C; k += 2) *reinterpret_cast<float2*>(rw + k) = make_float2(st.cur[k], st.cur[k + 1]);
            } else {
#pragma unroll
                for (int k = 0; k < C; ++k) rw[k] = st.cur[k];
            }
            float* own = row + st.jbase + lane_id();
#pragma unroll
            for (int i = 0; i < C; ++i)
                if (st.rd[i] >= 0) own[kWave * i] = st.rs[st.rd[i]];  // (nt stores: 25% slower)
        }
    }
};

}  // namespace wx

#endif  // WX_DP_FORWARD_H
