// wx_dp_config.h — what host and device share of the alignment DP (wx_align_dp.h): constants, cell
// layout, bucket tables, argument blocks, launchers.  All wx_align.hip needs to plan a launch; no kernel code.
#ifndef WX_DP_CONFIG_H
#define WX_DP_CONFIG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wx_align.h"
#include "wx_wave.h"  // kWave

namespace wx {

constexpr int kChunk = 32;  // emission rows per LDS buffer == bits per column word
constexpr int kUnroll = 8;  // time steps per unrolled group
constexpr int kMaxLdsFrames = 8192;  // segments up to this many frames keep walk state in LDS
constexpr int kGatherVS = 256;                      // compact row width (distinct columns)
constexpr int kMaxVocabWords = WX_MAX_VOCAB / 32;   // used-column bitmap words

// ------------------------------------------------------------------------------------
// Cell -> (lane, slot) layout of one segment.  G = ceil(N/C) lanes are used; the first
// n_short of them own C-1 cells, the rest C cells, so that column N always sits in the
// compile-time slot C-1 of lane G-1 (its value feeds the argmax every step without a
// dynamic register index).  Lanes >= G and the spare slot C-1 of short lanes compute
// harmless garbage: cells only ever feed cells to their right.
struct Layout {
    int C;        // cells per full lane
    int G;        // lanes used
    int n_short;  // leading lanes with C-1 cells
    int lanes;    // lanes of the workgroup (bitmap word stride)

    __host__ __device__ static Layout make(int C, int N, int lanes) {
        Layout L;
        L.C = C;
        L.lanes = lanes;
        L.G = (N + C - 1) / C;
        const int n_full = N - L.G * (C - 1);
        L.n_short = L.G - n_full;
        return L;
    }
    // first cell (1-based) and cell count of lane g
    __device__ __forceinline__ int first(int g) const {
        return g < n_short ? g * (C - 1) + 1 : n_short * (C - 1) + (g - n_short) * C + 1;
    }
    __device__ __forceinline__ int count(int g) const { return g < n_short ? C - 1 : (g < G ? C : 0); }
    // (lane, slot) of 0-based cell c; CC = C when known at compile time (0: runtime C)
    template <int CC = 0>
    __device__ __forceinline__ void locate(int c, int& g, int& k) const {
        const int Cc = CC > 0 ? CC : C;
        const int cs = n_short * (Cc - 1);
        if (c < cs) {
            g = Cc > 1 ? c / (Cc - 1) : 0;
            k = c - g * (Cc - 1);
        } else {
            const int c2 = c - cs;
            g = n_short + c2 / Cc;
            k = c2 - (g - n_short) * Cc;
        }
    }
};

// `waves` (virtual) waves of C cells per lane share a segment's columns with a chunk halo (Forward):
// every wave but the first spends its first halo_lanes on the >= kChunk cells before its own.  The one
// statement of that arithmetic: Geometry, bucket_capacity and split_capacity derive from it.
__host__ __device__ constexpr int halo_lanes(int C) { return (kChunk + C - 1) / C; }
__host__ __device__ constexpr int useful_lanes(int C, int waves) {
    return kWave + (waves - 1) * (kWave - halo_lanes(C));
}

template <int C, int W>
struct Geometry {
    static constexpr int HL = W > 1 ? halo_lanes(C) : 0;  // halo lanes per wave >= 1
    // useful lane index of (wave, lane); for a halo lane, the lane it mirrors
    __host__ __device__ static constexpr int lane_of(int wv, int l) {
        return wv == 0 ? l : kWave + (wv - 1) * (kWave - HL) + l - HL;
    }
    // (wave, lane) owning useful lane g
    __device__ static void owner(int g, int& wv, int& l) {
        if (g < kWave || W == 1) {
            wv = 0;
            l = g;
        } else {
            wv = 1 + (g - kWave) / (kWave - HL);
            l = HL + (g - kWave) % (kWave - HL);
        }
    }
};

constexpr int kMaxParts = 4;
// Column-N history: segment s at (row0 + kCnPad s) rounded down to 16 bytes, so at least
// kCnPad - 3 floats past its T rows are its own: the register-resident owner stores all four
// 8-row groups of a partial last chunk, up to 31 rows past T.
constexpr int kCnPad = 40;
constexpr int kXcdStride = 8;  // blocks b and b + 8 share an XCD (MI355X: 8 XCDs, round-robin)
__host__ __device__ constexpr unsigned split_grid(int S, int P) {
    return (unsigned)((S + kXcdStride - 1) / kXcdStride * kXcdStride * P);
}
constexpr int kHaloCells = 40;  // >= HL * C = ceil(32 / C) * C for every C
constexpr int kMaxSpin = 1 << 16;

constexpr int kArgFenced = 1;     // AlignArgs::flags: release/acquire at the split arrival
constexpr int kArgXcdSpread = 2;  // AlignArgs::flags: parts of a segment on different XCDs (tests)

// (cells per lane C, DP waves per segment W, helper wave H) buckets, one kernel
// instantiation each; id = C << 8 | W << 1 | H.
// Throughput mode (many segments in flight): one wave per segment up to N = 512; longer
// transcripts use W waves of 8 cells per lane with a chunk halo (Geometry): at most ~124
// VGPRs keeps 4 waves per SIMD, which beat one wide (16-32 cells per lane) wave per
// segment by 4-10% on T = 3000, N = 900 batches.  Latency mode (few segments: the
// chip would otherwise be mostly idle): a segment's columns are spread over 3 or 7 waves
// plus the helper (at most 2 waves per SIMD, which still issue at the full rate), so each
// wave issues fewer instructions per time step.  (Waves beyond column N only keep the
// barrier count, so a wide bucket costs no time: 30 s segments, N 257..704, share one.)
#define WX_BUCKETS(X)                                                                                    \
    X(1, 1, 0) X(2, 1, 0) X(4, 1, 0) X(6, 1, 0) X(8, 1, 0) X(8, 2, 0) X(8, 4, 0) X(8, 8, 0) X(16, 8, 0) \
        X(32, 8, 0) X(1, 3, 1) X(1, 7, 1) X(2, 7, 1) X(4, 7, 1) X(8, 7, 1)

__host__ __device__ constexpr int bucket_make(int C, int W, int H) { return (C << 8) | (W << 1) | H; }
__host__ __device__ constexpr int bucket_C(int id) { return id >> 8; }
__host__ __device__ constexpr int bucket_W(int id) { return (id >> 1) & 127; }

__host__ __device__ constexpr int bucket_capacity(int C, int W) { return C * useful_lanes(C, W); }  // max N

// Buckets of each mode in increasing capacity, (32, 8, 0) after both (compare chains: a
// dynamically indexed table would live in scratch on the device).
#define WX_CHAIN_THROUGHPUT(X) \
    X(1, 1, 0) X(2, 1, 0) X(4, 1, 0) X(6, 1, 0) X(8, 1, 0) X(8, 2, 0) X(8, 4, 0) X(8, 8, 0) X(16, 8, 0)
#define WX_CHAIN_LATENCY(X) X(1, 1, 0) X(1, 3, 1) X(1, 7, 1) X(2, 7, 1) X(4, 7, 1) X(8, 7, 1) X(16, 8, 0)
#define WX_PICK(CC, WW, HH) \
    if (N <= bucket_capacity(CC, WW)) return bucket_make(CC, WW, HH);
__host__ __device__ __forceinline__ constexpr int bucket_id(int N, int mode = 0) {
    if (mode == 1) {
        WX_CHAIN_LATENCY(WX_PICK)
    } else {
        WX_CHAIN_THROUGHPUT(WX_PICK)
    }
    return bucket_make(32, 8, 0);
}
#undef WX_PICK

// bitmap words per 32-step block of a segment in bucket `id`
__host__ __device__ __forceinline__ int bucket_cells_total(int id) { return bucket_C(id) * kWave * bucket_W(id); }

// Split buckets (C cells per lane, W DP waves + 1 helper per part, P parts): the chunk
// halo runs through all W * P virtual waves.  Segments too long for the widest split bucket
// use the single-CU latency buckets in the same launch.
// (A/B, config 2: 5 DP waves per part instead of 4 were 2 us slower, 6 — two hand-off hops
// fewer — 0.8 us faster, though the DP waves sharing a SIMD slow each other's chains.)
#define WX_SPLIT_BUCKETS(X) X(1, 3) X(1, 4) X(2, 3) X(4, 3)
constexpr int kSplitFlag = 1 << 20;
__host__ __device__ constexpr int split_capacity(int C, int W, int P) { return C * useful_lanes(C, W * P); }
#define WX_PICK_SPLIT(CC, WW) \
    if (N <= split_capacity(CC, WW, P)) return bucket_make(CC, WW, 1) | kSplitFlag;
__host__ __device__ __forceinline__ constexpr int split_bucket_id(int N, int P) {
    WX_SPLIT_BUCKETS(WX_PICK_SPLIT)
    return bucket_id(N, 1);
}
#undef WX_PICK_SPLIT

// A split launch runs ONE split kernel (the bucket of the batch's longest segment): its
// grid is S * P workgroups, one per CU, and a second split grid would queue behind it
// (measured: workgroups of the second kernel started up to 70 us late).  Shorter segments
// leave that bucket's extra waves idle.  Segments beyond its capacity use the single-CU
// latency buckets.
__host__ __device__ __forceinline__ constexpr int split_capacity_of(int id, int P) {
    return split_capacity(bucket_C(id & ~kSplitFlag), bucket_W(id & ~kSplitFlag), P);
}
// Layout::make needs N >= ceil(N/C) * (C-1) (at most one missing cell per lane); the
// per-N buckets always satisfy it, a launch-wide split bucket may not for short segments,
// which then take a throughput bucket (one wave, small LDS: it shares CUs with the parts).
__host__ __device__ constexpr bool layout_fits(int N, int C) { return N >= (N + C - 1) / C * (C - 1); }
__host__ __device__ __forceinline__ int launch_split_bucket(int N, int P, int split_id) {
    if (N > split_capacity_of(split_id, P)) return bucket_id(N, 1);
    return layout_fits(N, bucket_C(split_id & ~kSplitFlag)) ? split_id : bucket_id(N, 0);
}

// The tables against Geometry: a bucket's capacity ends at the last lane of its last (virtual) wave, a part's
// halo fits its granule block; each chain's capacities strictly increase (a bucket out of order is never picked).
template <int K>
constexpr bool increasing(const int (&a)[K]) {
    for (int i = 0; i + 1 < K; ++i)
        if (a[i] >= a[i + 1]) return false;
    return true;
}
#define WX_CAP(CC, WW, HH) bucket_capacity(CC, WW),
static_assert(increasing({WX_CHAIN_THROUGHPUT(WX_CAP) bucket_capacity(32, 8)}) &&
                  increasing({WX_CHAIN_LATENCY(WX_CAP) bucket_capacity(32, 8)}), "bucket_id: capacities must increase");
#undef WX_CAP
#define WX_CAP(CC, WW) split_capacity(CC, WW, P),
constexpr bool split_increasing(int P) { return increasing({WX_SPLIT_BUCKETS(WX_CAP)}); }
#undef WX_CAP
static_assert(split_increasing(2) && split_increasing(3) && split_increasing(4), "split_bucket_id: capacities must increase");
#define WX_CHECK(CC, WW, HH)                                                                           \
    static_assert(bucket_capacity(CC, WW) == CC * (Geometry<CC, WW>::lane_of(WW - 1, kWave - 1) + 1), \
                  "bucket_capacity disagrees with Geometry");
WX_BUCKETS(WX_CHECK)
#undef WX_CHECK
#define WX_CHECK_P(CC, WW, P) (split_capacity(CC, WW, P) == CC * (Geometry<CC, 2>::lane_of(WW * P - 1, kWave - 1) + 1))
#define WX_CHECK(CC, WW)                                                                                   \
    static_assert(WX_CHECK_P(CC, WW, 2) && WX_CHECK_P(CC, WW, 3) && WX_CHECK_P(CC, WW, 4),                 \
                  "split_capacity disagrees with Geometry");                                               \
    static_assert(CC * Geometry<CC, 2>::HL <= kHaloCells, "a part's halo must fit its granule block");
WX_SPLIT_BUCKETS(WX_CHECK)
#undef WX_CHECK
#undef WX_CHECK_P

struct AlignArgs {
    const float* em;
    const int64_t* em_off;
    int V;
    const int32_t* tok;
    const int64_t* tok_off;
    const int32_t* blank_id;
    int S;
    int mode;  // 0 throughput buckets, 1 latency buckets
    int x4;    // V == 32 and 16-byte aligned rows: 16-byte LDS staging
    int32_t* seg_start;
    int32_t* seg_end;
    double* seg_score;
    int32_t* t_start;
    int32_t* status;
    unsigned* bits;  // workspace: bitmap region
    int bits_stride_cells;  // 64 * Cstride dwords per block
    float* q0;       // workspace: sum_T floats
    unsigned* cmask; // workspace: walk change masks, (floor(row0/32) + seg) words per segment
    double* c0acc;   // workspace (MODE 2): column-0 fp64 cumsum per chunk, same offsets as cmask
    float* cn;       // workspace: column N history, segment at (row0 + 4 seg) & ~3
    int parts;       // split launches: workgroups (CUs) per segment, else 1
    int split_id;    // split launches: the one split bucket (segments up to its capacity)
    unsigned epoch;  // split launches: per-launch tag of the hand-off granules and counters
    uint64_t* xg;    // workspace: hand-off granules, (floor(row0/32) + seg + q) * 3 * 40
    uint64_t* arrive;// workspace: per-segment arrival counters {count, epoch} (split_arrive)
    int spin;        // split launches: hand-off re-reads before a part counts as lost
    int flags;       // split launches: kArgFenced | kArgXcdSpread (WX_SPLIT_FENCED, WX_SPLIT_XCD_SPREAD)
};

struct TrellisArgs {
    const float* em;
    const int64_t* em_off;
    int V;
    const int32_t* tok;
    const int64_t* tok_off;
    const int32_t* blank_id;
    float* tr;
    const int64_t* tr_off;
    int x4;
};

// Development builds for A/B timing of V <= 32 batches (tools/ab): -DWX_DEV_V32 instantiates
// the V <= 32 kernels only (a third of the compile time); wider vocabularies are NOT served.
#ifdef WX_DEV_V32
#define WX_VS64 32
#define WX_VSG 32
#else
#define WX_VS64 64
#define WX_VSG kGatherVS
#endif

// Launchers of the kernel templates (wx_align_dp.h).  Each instantiation is compiled in one of the
// shards of wx_align_inst.hip (explicit instantiations, built in parallel); the host ABI in
// wx_align.hip only references them.
template <int C, int VS, int W, int H>
void launch_align_dp(dim3 grid, hipStream_t s, const AlignArgs& a);
template <int C, int VS, int W>
void launch_align_split(dim3 grid, hipStream_t s, const AlignArgs& a);
template <int C, int VS, int W>
void launch_trellis(dim3 grid, hipStream_t s, const TrellisArgs& a);

}  // namespace wx

#endif  // WX_DP_CONFIG_H
