// wx_align.hip — the alignment's host C ABI (include/wx_align.h) and its non-template kernels
// (materialised-trellis backtrack, merge_repeats, column-0 cumsum).  The fused DP and
// get_trellis kernel templates live in wx_align_dp.h and its wx_dp_*.h (this file includes only
// what plans a launch and what backtrack_kernel shares with them); their instantiations are
// compiled in the shards of wx_align_inst.hip.  Every other stage has a file of its own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>

#include "wx_dp_config.h"
#include "wx_dp_prims.h"
#include "wx_dp_tail.h"
#include "wx_dp_walk.h"
#include "wx_host.h"
#ifdef WX_PHASE_TIMING  // one TU: the phase-timing device arrays must be a single copy
#include "wx_align_inst.hip"
#endif

#define WX_VERSION "0.1.0"

namespace wx {

// ------------------------------------------------------------------------------------
// backtrack() from a materialised trellis: recompute the decision bits from the trellis
// (one column word per thread: 32 rows of one cell), argmax of column N, shared walk,
// then expand the per-token spans into the reference's Point list.
struct BacktrackArgs {
    const float* tr;
    const int64_t* tr_off;
    const float* em;
    const int64_t* em_off;
    int V;
    const int32_t* tok;
    const int64_t* tok_off;
    const int32_t* blank_id;
    int32_t* path_tok;
    int32_t* path_time;
    float* path_prob;
    int32_t* path_len;
    int32_t* t_start;
    unsigned* bits;
    int bits_stride_cells;
    int32_t* start;  // workspace: per-token start frames (CSR by tok_off)
    unsigned* cmask; // workspace: walk change masks
};

__global__ __launch_bounds__(256) void backtrack_kernel(BacktrackArgs a) {
    const int seg = blockIdx.x;
    const SegDesc d = load_desc(a.em_off, a.tok_off, a.blank_id, seg);
    const int T = d.T, N = d.N;
    const float* tr = a.tr + a.tr_off[seg];
    const float* E = a.em + d.row0 * a.V;
    const int32_t* tok = a.tok + d.tok0;
    const int64_t W = (int64_t)N + 1;
    const int cpl = max(1, (N + kWave - 1) / kWave);
    unsigned* bits = a.bits + ((d.row0 >> 5) + seg) * (int64_t)a.bits_stride_cells;
    const int nblk = (T + kChunk - 1) / kChunk;
    // (1) decision words: word (b, cell j) bit 31-s = changed>stayed at decision u = 32b+s
    const int nwords = nblk * cpl * kWave;
    for (int i = threadIdx.x; i < nwords; i += blockDim.x) {
        const int g = i % kWave;
        const int k = (i / kWave) % cpl;
        const int b = i / (kWave * cpl);
        const int j = g * cpl + k + 1;
        unsigned wv = 0u;
        if (j <= N) {
            int tk = tok[j - 1];
            tk = (tk >= 0 && tk < a.V) ? tk : 0;
            for (int s = 0; s < kChunk; ++s) {
                const int u = b * kChunk + s;
                unsigned bit = 0u;
                if (u < T) {
                    const float stayed = tr[(int64_t)u * W + j] + E[(int64_t)u * a.V + d.blank];
                    const float changed = tr[(int64_t)u * W + j - 1] + E[(int64_t)u * a.V + tk];
                    bit = changed > stayed ? 1u : 0u;
                }
                wv = (wv << 1) | bit;
            }
        }
        bits[((int64_t)b * cpl + k) * kWave + g] = wv;
    }
    // (2) argmax of column N over rows 0..T (first max, NaN counts as max)
    __shared__ float sv[256];
    __shared__ int si[256];
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    bool bn = false;
    for (int t = threadIdx.x; t <= T; t += blockDim.x) {
        const float v = tr[(int64_t)t * W + N];
        if (bn) continue;
        if (v != v) {
            bn = true;
            bv = v;
            bi = t;
        } else if (bi == 0x7fffffff || v > bv) {
            bv = v;
            bi = t;
        }
    }
    sv[threadIdx.x] = bn ? NAN : bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int off = blockDim.x / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const float v1 = sv[threadIdx.x], v2 = sv[threadIdx.x + off];
            const int i1 = si[threadIdx.x], i2 = si[threadIdx.x + off];
            const bool n1 = v1 != v1 && i1 != 0x7fffffff, n2 = v2 != v2 && i2 != 0x7fffffff;
            bool take2;
            if (i2 == 0x7fffffff) take2 = false;
            else if (i1 == 0x7fffffff) take2 = true;
            else if (n1 && n2) take2 = i2 < i1;
            else if (n1) take2 = false;
            else if (n2) take2 = true;
            else if (v2 > v1) take2 = true;
            else if (v1 > v2) take2 = false;
            else take2 = i2 < i1;
            if (take2) {
                sv[threadIdx.x] = v2;
                si[threadIdx.x] = i2;
            }
        }
        __syncthreads();
    }
    const int ts = (N == 0) ? 0 : si[0];
    if (threadIdx.x == 0) a.t_start[seg] = ts;
    __threadfence_block();
    __syncthreads();
    // (3) walk (wave 0)
    int32_t* start = a.start + d.tok0;
    __shared__ int ok_sh;
    if (threadIdx.x < kWave) {
        Layout lay;
        lay.C = cpl;
        lay.G = kWave;
        lay.n_short = 0;
        lay.lanes = kWave;
        unsigned* cmask = a.cmask + ((d.row0 >> 5) + seg);
        const int b_lo = walk<0>(bits, lay, N, ts, cmask, false);
        if (b_lo >= 0) {
            wave_fence();
            compact_starts(cmask, b_lo, (ts - 1) >> 5, start);
        }
        const bool ok = b_lo >= 0;
        if (threadIdx.x == 0) ok_sh = ok ? 1 : 0;
    }
    wait_vm();
    block_fence();
    const bool ok = ok_sh != 0;
    if (threadIdx.x == 0) a.path_len[seg] = ok ? (ts - start[0]) : -1;
    if (!ok) return;
    // (4) expand spans -> Points (forward order) at path offset em_off[seg]
    const int base_t = start[0];
    int32_t* ptok = a.path_tok + d.row0;
    int32_t* ptime = a.path_time + d.row0;
    float* pprob = a.path_prob + d.row0;
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        const int s = start[k];
        const int e = (k + 1 < N) ? start[k + 1] : ts;
        int tk = tok[k];
        tk = (tk >= 0 && tk < a.V) ? tk : 0;
        for (int x = s; x < e; ++x) {
            ptok[x - base_t] = k;
            ptime[x - base_t] = x;
            pprob[x - base_t] = exp_cr(E[(int64_t)x * a.V + (x == s ? tk : 0)]);
        }
    }
}

// ------------------------------------------------------------------------------------
// merge_repeats over arbitrary paths: run boundaries by ballot, then one fp64 left-to-right
// sum per run.  One wave per path.
struct MergeArgs {
    const int32_t* ptok;
    const int32_t* ptime;
    const float* pprob;
    const int64_t* path_off;
    const int32_t* path_len;
    int32_t* seg_tok;
    int32_t* seg_start;
    int32_t* seg_end;
    double* seg_score;
    int32_t* seg_count;
};

__global__ __launch_bounds__(kWave) void merge_repeats_kernel(MergeArgs a) {
    const int seg = blockIdx.x;
    const int lane = lane_id();
    const int L = uniform(a.path_len[seg]);
    if (L <= 0) {
        if (lane == 0) a.seg_count[seg] = 0;
        return;
    }
    const int64_t off = a.path_off[seg];
    const int32_t* pt = a.ptok + off;
    const int32_t* pm = a.ptime + off;
    const float* pp = a.pprob + off;
    int32_t* gstart = a.seg_end + off;  // scratch: run start indices, overwritten below
    int G = 0;
    for (int i0 = 0; i0 < L; i0 += kWave) {
        const int i = i0 + lane;
        bool flag = false;
        if (i < L) flag = (i == 0) || (pt[i] != pt[i - 1]);
        const unsigned long long m = __ballot(flag);
        const int pos = G + __popcll(m & ((1ull << lane) - 1ull));
        if (flag) gstart[pos] = i;
        G += __popcll(m);
    }
    wait_vm();
    block_fence();
    for (int g0 = 0; g0 < G; g0 += kWave) {
        const int g = g0 + lane;
        int i1 = 0, i2 = 0;
        if (g < G) {
            i1 = gstart[g];
            i2 = (g + 1 < G) ? gstart[g + 1] : L;
        }
        wait_vm();
        block_fence();
        if (g < G) {
            double sum = 0.0;
            for (int i = i1; i < i2; ++i) sum += (double)pp[i];
            a.seg_tok[off + g] = pt[i1];
            a.seg_start[off + g] = pm[i1];
            a.seg_end[off + g] = pm[i2 - 1] + 1;
            a.seg_score[off + g] = sum / (double)(i2 - i1);
        }
        wait_vm();
        block_fence();
    }
    if (lane == 0) a.seg_count[seg] = G;
}

// Column 0 of get_trellis (alignment.py:367): S(t) = em[0, c] + ... + em[t - 1, c] in double,
// row order, t = 0..T — the fused DP's own column-0 routine (col0_chunk: the sequential chain,
// one EXEC-masked fp64 add per row), one wave.  Rows past T in the last chunk enter as 0 and
// feed only sums past S(T), which are not stored.
__global__ __launch_bounds__(kWave) void column0_cumsum_kernel(const float* __restrict__ em, int64_t T, int V,
                                                               double* __restrict__ S) {
    const int l = lane_id();
    double acc = 0.0;
    for (int64_t t0 = 0; t0 < T; t0 += kChunk) {
        const int64_t t = t0 + (l & (kChunk - 1));
        const float e = t < T ? em[t * V] : 0.0f;
        const double a = col0_chunk(acc, e);
        // S(t0 + l) for the chunk's rows that exist: the last chunk may be partial, and its lanes
        // at and past T hold sums the header does not promise room for
        if (l < kChunk && t0 + l < T) S[t0 + l] = a;
    }
    if (l == 0) S[T] = acc;  // S(T): the sum over every row (the rows past T entered as 0)
}
}  // namespace wx

// ======================================================================================
// C ABI
using namespace wx;

namespace {

// Kernels of different (C, W) buckets are independent: a batch that spans several buckets
// forks them onto a small per-device pool of non-blocking streams and joins back onto the
// caller's stream with events, so they run concurrently (a latency-bound batch then costs
// the slowest bucket, not their sum).  Created once per device; enqueue is serialised by
// a mutex so concurrent callers cannot interleave fork/join events.
struct ForkPool {
    static constexpr int kMax = 12;
    hipStream_t s[kMax];
    hipEvent_t fork;
    hipEvent_t join[kMax];
    std::mutex mu;
};

ForkPool* fork_pool() {
    static std::mutex mu;
    static ForkPool* pools[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    if (!pools[dev]) {
        ForkPool* p = new ForkPool;
        bool ok = hipEventCreateWithFlags(&p->fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; ok && i < ForkPool::kMax; ++i) {
            ok = hipStreamCreateWithFlags(&p->s[i], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&p->join[i], hipEventDisableTiming) == hipSuccess;
        }
        if (!ok) return nullptr;
        pools[dev] = p;
    }
    return pools[dev];
}

// Run launch(i, stream) for i in [0, n): on the caller's stream when n == 1, otherwise
// forked over the pool and joined back onto `st`.
template <class F>
int fork_join(hipStream_t st, int n, F&& launch) {
    if (n <= 0) return WX_OK;
    ForkPool* p = n > 1 && n <= ForkPool::kMax ? fork_pool() : nullptr;
    if (!p) {  // one launch, or no pool: serially on the caller's stream
        for (int i = 0; i < n; ++i) launch(i, st);
        return launch_status();
    }
    std::lock_guard<std::mutex> g(p->mu);
    hipError_t e = hipEventRecord(p->fork, st);
    for (int i = 0; i < n && e == hipSuccess; ++i) {
        e = hipStreamWaitEvent(p->s[i], p->fork, 0);
        if (e != hipSuccess) break;
        launch(i, p->s[i]);
        e = hipEventRecord(p->join[i], p->s[i]);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, p->join[i], 0);
    }
    const int rc = launch_status();
    return e != hipSuccess ? (int)e : rc;
}

// bucket ids in launch order, ids = C*64 + W
constexpr int kBucketIds[] = {
#define WX_ID(CC, WW, HH) bucket_make(CC, WW, HH),
    WX_BUCKETS(WX_ID)
#undef WX_ID
};
constexpr int kNumBuckets = sizeof(kBucketIds) / sizeof(int);

// The buckets that segments with N in [min_N, max_N] map to (N == 0 -> the first one).
int buckets_for(int64_t min_N, int64_t max_N, int mode, int* ids) {
    int n = 0;
    int64_t N = std::max<int64_t>(min_N, 1);
    const int64_t hi = std::max<int64_t>(max_N, 1);
    while (N <= hi) {
        const int id = bucket_id((int)N, mode);
        ids[n++] = id;
        N = (int64_t)bucket_capacity(bucket_C(id), bucket_W(id)) + 1;
    }
    return n;
}

// The split launch's one split bucket, for a batch whose longest segment has max_N tokens.
int split_launch_id(int64_t max_N, int P) {
    const int id = split_bucket_id((int)std::min<int64_t>(std::max<int64_t>(max_N, 1), 1 << 20), P);
    if (id & kSplitFlag) return id;
    int widest = 0;
#define WX_WIDEST(CC, WW) widest = bucket_make(CC, WW, 1) | kSplitFlag;
    WX_SPLIT_BUCKETS(WX_WIDEST)
#undef WX_WIDEST
    return widest;
}

// Kernels of a split launch: the split bucket, then the single-CU latency buckets of any
// segment too long for it.
int buckets_for_split(int64_t min_N, int64_t max_N, int P, int split_id, int* ids) {
    int n = 0;
    ids[n++] = split_id;
    const int64_t cap = split_capacity_of(split_id, P);
    const int C = bucket_C(split_id & ~kSplitFlag);
    const int64_t small_hi = std::min<int64_t>(max_N, (int64_t)C * (C - 1));  // layout_fits holds above
    if (C > 2 && min_N <= small_hi) n += buckets_for(min_N, small_hi, WX_MODE_THROUGHPUT, ids + n);
    if (max_N > cap) n += buckets_for(std::max<int64_t>(min_N, cap + 1), max_N, WX_MODE_LATENCY, ids + n);
    return n;
}

// bitmap words per block of the bucket `id` of an N-token segment in a launch of P parts
int launch_cells_total(int id, int P) {
    return (id & kSplitFlag) ? bucket_cells_total(id & ~kSplitFlag) * P : bucket_cells_total(id);
}

// The hand-off region of split launches, inside the DP workspace or the caller's own:
// granules per (floor(row0/32) + seg + chunk) block, 3 boundaries x 40, then the arrival words.
size_t carve_handoff(Carver& c, int32_t S, int64_t sum_T, AlignArgs& a) {
    a.xg = c.take<uint64_t>((size_t)(sum_T / kChunk + S + 2) * (kMaxParts - 1) * kHaloCells);
    a.arrive = c.take<uint64_t>((size_t)(S + 1));
    return c.off;
}

// The DP workspace: the one statement of its layout (the size query measures it on a null base).
size_t carve_dp(Carver& c, int32_t S, int64_t sum_T, int64_t max_N, AlignArgs& a) {
    const int nmax = (int)std::max<int64_t>(max_N, 1);  // widest bucket of any launch shape
    int cells = std::max(bucket_cells_total(bucket_id(nmax, 0)), bucket_cells_total(bucket_id(nmax, 1)));
    for (int P = 2; P <= kMaxParts; ++P) cells = std::max(cells, launch_cells_total(split_launch_id(nmax, P), P));
    const int64_t blocks = sum_T / kChunk + S + 1;
    // bitmap: per segment (floor(row0/32) + seg) block offsets, 64 * C_stride dwords per block
    a.bits_stride_cells = cells;
    a.bits = c.take<unsigned>((size_t)blocks * (size_t)cells);
    a.q0 = c.take<float>((size_t)(sum_T + 1));
    a.cmask = c.take<unsigned>((size_t)blocks);
    a.cn = c.take<float>((size_t)(sum_T + kCnPad * (int64_t)S + 16));  // column N: segment s at (row0 + 4 s) & ~3
    a.c0acc = c.take<double>((size_t)(blocks + 1));  // checkpointed kernels' column-0 cumsum per chunk (+ seg + q)
    return carve_handoff(c, S, sum_T, a);  // its own hand-off region: used when the caller passes none
}

// The backtrack workspace: bitmap, per-token start frames (sum of N <= S * max_N), chunk mask.
size_t carve_backtrack(Carver& c, int32_t S, int64_t sum_T, int64_t max_N, BacktrackArgs& a) {
    const int64_t cpl = std::max<int64_t>(1, (max_N + kWave - 1) / kWave);
    const int64_t blocks = sum_T / kChunk + S + 1;
    a.bits_stride_cells = (int)(kWave * cpl);
    a.bits = c.take<unsigned>((size_t)blocks * kWave * (size_t)cpl);
    a.start = c.take<int32_t>((size_t)(S * max_N + 1));
    a.cmask = c.take<unsigned>((size_t)blocks);
    return c.off;
}

}  // namespace

extern "C" {

const char* wx_version(void) { return WX_VERSION " gfx950"; }

const char* wx_strerror(int code) {
    switch (code) {
        case WX_OK: return "ok";
        case WX_E_INVALID: return "invalid argument";
        case WX_E_VOCAB: return "vocabulary size outside [1, 16384]";
        case WX_E_TOO_LONG: return "segment has more than 16000 tokens";
        case WX_E_WORKSPACE: return "workspace too small";
        case WX_E_LAUNCH: return "kernel launch failed";
        default: return hipGetErrorString((hipError_t)code);
    }
}

// Launch shape: latency buckets while the batch cannot fill the chip with one wave per
// segment.  WX_ALIGN_MODE=0/1 forces a shape for WX_MODE_AUTO calls (benchmarking only).
int align_mode(int32_t S, int32_t mode) {
    if (mode == WX_MODE_THROUGHPUT) return mode;
    if (mode != WX_MODE_AUTO) return WX_MODE_LATENCY;  // LATENCY, LATENCY_1CU, SPLIT2..4
    static const int forced = [] {
        const char* e = getenv("WX_ALIGN_MODE");
        return (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : -1;
    }();
    if (forced >= 0) return forced;
    return S <= 256 ? WX_MODE_LATENCY : WX_MODE_THROUGHPUT;
}

size_t wx_align_dp_workspace_bytes(int32_t S, int64_t sum_T, int64_t max_N) {
    Carver c{nullptr};
    AlignArgs a;
    return carve_dp(c, S, sum_T, max_N, a);
}

// CUs of the current device (cached per device).
int device_cus() {
    static int cache[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cache[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cache[dev] = n;
    }
    return cache[dev];
}

// Parts per segment of a latency launch.  WX_MODE_AUTO splits each segment over 4 CUs when
// the device has 4 CUs per segment (S <= 64 on MI355X), else one CU; WX_MODE_LATENCY is one CU
// unless WX_PARTS=2..4 asks for a split; WX_MODE_SPLIT2..4 ask explicitly.  Measured (T=1499
// and T=2999 segments, round 1): 4 parts take 90 / 101 / 210 us for 16 x 1499 / 64 x 1499 /
// 64 x 2999 against 107 / 110 / 309 us on one CU; 2 or 3 parts gain nothing (they pick C=2
// buckets, whose step is as long as the one-CU bucket's).  Every part stages all emission
// rows (4x the emission reads, ~0.5 TB/s at config 2: far from any bound).  The CU count
// caps the parts: part p only waits for part p-1, which the dispatcher starts first.
int split_parts(int32_t S, int mode, int32_t requested) {
    static const int forced = [] {
        const char* e = getenv("WX_PARTS");
        return (e && e[0] >= '1' && e[0] <= '0' + kMaxParts) ? e[0] - '0' : 0;
    }();
    if (mode != WX_MODE_LATENCY) return 1;
    if (requested == WX_MODE_LATENCY_1CU) return 1;
    const int fit = device_cus() / std::max(S, 1);
    int want = 1;
    if (requested >= WX_MODE_SPLIT2 && requested <= WX_MODE_SPLIT4)
        want = requested - WX_MODE_SPLIT2 + 2;
    else if (forced)
        want = forced;
    else if (requested == WX_MODE_AUTO && fit >= kMaxParts)
        want = kMaxParts;
    if (want <= 1) return 1;
    return std::max(1, std::min(want, fit)) >= 2 ? std::max(1, std::min(want, fit)) : 1;
}

unsigned next_epoch() {  // never 0: a zeroed granule or counter carries no valid tag
    static std::atomic<unsigned> e{(unsigned)std::chrono::steady_clock::now().time_since_epoch().count()};
    const unsigned v = e.fetch_add(1) + 1;
    return v ? v : 1u;
}

// Hand-off re-reads before a split part gives up on a granule.  WX_SPIN_LIMIT (read per call)
// lowers it; 0 forces every consumer to lose its hand-offs (the recovery test).
static int spin_limit() {
    const char* e = getenv("WX_SPIN_LIMIT");
    if (e && e[0] >= '0' && e[0] <= '9') return std::min(atoi(e), kMaxSpin);
    return kMaxSpin;
}
// Split-arrival flags, read per call (tests and A/B): WX_SPLIT_FENCED=1 adds the release /
// acquire fences to the write-through arrival, WX_SPLIT_XCD_SPREAD=1 spreads each segment's
// parts over different XCDs.
static int split_flags() {
    auto on = [](const char* n) {
        const char* e = getenv(n);
        return e && e[0] == '1';
    };
    return (on("WX_SPLIT_FENCED") ? kArgFenced : 0) | (on("WX_SPLIT_XCD_SPREAD") ? kArgXcdSpread : 0);
}

size_t wx_align_dp_handoff_bytes(int32_t S, int64_t sum_T) {
    Carver c{nullptr};
    AlignArgs a;
    return carve_handoff(c, S, sum_T, a);
}

int wx_align_dp(const float* em, const int64_t* em_off, int32_t V, const int32_t* tok, const int64_t* tok_off,
                const int32_t* blank_id, int32_t S, int64_t min_N, int64_t max_N, int64_t sum_T, int32_t* seg_start,
                int32_t* seg_end, double* seg_score, int32_t* t_start, int32_t* status, void* workspace,
                size_t workspace_bytes, void* stream) {
    return wx_align_dp_mode(em, em_off, V, tok, tok_off, blank_id, S, min_N, max_N, sum_T, seg_start, seg_end,
                            seg_score, t_start, status, workspace, workspace_bytes, WX_MODE_AUTO, stream);
}

int wx_align_dp_mode(const float* em, const int64_t* em_off, int32_t V, const int32_t* tok,
                     const int64_t* tok_off, const int32_t* blank_id, int32_t S, int64_t min_N, int64_t max_N,
                     int64_t sum_T, int32_t* seg_start, int32_t* seg_end, double* seg_score, int32_t* t_start,
                     int32_t* status, void* workspace, size_t workspace_bytes, int32_t mode, void* stream) {
    return wx_align_dp_ex(em, em_off, V, tok, tok_off, blank_id, S, min_N, max_N, sum_T, seg_start, seg_end,
                          seg_score, t_start, status, workspace, workspace_bytes, nullptr, 0, mode, stream);
}

int wx_align_dp_ex(const float* em, const int64_t* em_off, int32_t V, const int32_t* tok,
                   const int64_t* tok_off, const int32_t* blank_id, int32_t S, int64_t min_N, int64_t max_N,
                   int64_t sum_T, int32_t* seg_start, int32_t* seg_end, double* seg_score, int32_t* t_start,
                   int32_t* status, void* workspace, size_t workspace_bytes, void* handoff, size_t handoff_bytes,
                   int32_t mode, void* stream) {
    if (!(mode >= WX_MODE_AUTO && mode <= WX_MODE_LATENCY_1CU) && !(mode >= WX_MODE_SPLIT2 && mode <= WX_MODE_SPLIT4))
        return WX_E_INVALID;
    if (S < 0 || sum_T < 0 || min_N < 0 || max_N < min_N) return WX_E_INVALID;
    if (S == 0) return WX_OK;
    if (!em || !em_off || !tok_off || !blank_id || !seg_start || !seg_end || !seg_score || !t_start || !status ||
        !workspace)
        return WX_E_INVALID;
    if (V < 1 || V > WX_MAX_VOCAB) return WX_E_VOCAB;
#ifdef WX_DEV_V32
    if (V > 32) return WX_E_INVALID;  // development build: only the V <= 32 kernels exist
#endif
    if (max_N > WX_MAX_TOKENS) return WX_E_TOO_LONG;
    AlignArgs a;
    Carver ws{workspace}, ho{handoff};  // (the caller's hand-off region takes the place of the workspace's)
    if (workspace_bytes < carve_dp(ws, S, sum_T, max_N, a)) return WX_E_WORKSPACE;
    if (handoff && handoff_bytes < carve_handoff(ho, S, sum_T, a)) return WX_E_WORKSPACE;
    a.em = em; a.em_off = em_off; a.V = V; a.tok = tok; a.tok_off = tok_off; a.blank_id = blank_id; a.S = S;
    a.seg_start = seg_start; a.seg_end = seg_end; a.seg_score = seg_score; a.t_start = t_start; a.status = status;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    a.mode = align_mode(S, mode);
    a.parts = split_parts(S, a.mode, mode);
    a.epoch = next_epoch();
    a.spin = spin_limit();
    a.flags = split_flags();
    if (a.parts > 1 && !handoff) {  // workspace hand-off region: holds anything until zeroed
        const hipError_t e = hipMemsetAsync(a.xg, 0, wx_align_dp_handoff_bytes(S, sum_T), st);
        if (e != hipSuccess) return (int)e;
    }
    a.x4 = (V == 32 && (reinterpret_cast<uintptr_t>(em) & 15) == 0) ? 1 : 0;
    int ids[kNumBuckets + 8];
    a.split_id = a.parts > 1 ? split_launch_id(max_N, a.parts) : 0;
    const int n = a.parts > 1 ? buckets_for_split(min_N, max_N, a.parts, a.split_id, ids)
                              : buckets_for(min_N, max_N, a.mode, ids);
    const dim3 grid(S);
    return fork_join(st, n, [&](int i, hipStream_t s) {
#define WX_LAUNCH_SPLIT(CC, WW)                                                                        \
        if (ids[i] == (bucket_make(CC, WW, 1) | kSplitFlag)) {                                          \
            const dim3 g2(split_grid(S, a.parts));                                                        \
            if (V <= 32) launch_align_split<CC, 32, WW>(g2, s, a);                                         \
            else if (V <= 64) launch_align_split<CC, WX_VS64, WW>(g2, s, a);                                \
            else launch_align_split<CC, WX_VSG, WW>(g2, s, a);                                            \
        }
        WX_SPLIT_BUCKETS(WX_LAUNCH_SPLIT)
#undef WX_LAUNCH_SPLIT
#define WX_LAUNCH_ALIGN(CC, WW, HH)                                                                  \
        if (ids[i] == bucket_make(CC, WW, HH)) {                                                       \
            if (V <= 32) launch_align_dp<CC, 32, WW, HH>(grid, s, a);                                  \
            else if (V <= 64) launch_align_dp<CC, WX_VS64, WW, HH>(grid, s, a);                             \
            else launch_align_dp<CC, WX_VSG, WW, HH>(grid, s, a);                                   \
        }
        WX_BUCKETS(WX_LAUNCH_ALIGN)
#undef WX_LAUNCH_ALIGN
    });
}

int wx_align_dp_plan(int32_t S, int64_t min_N, int64_t max_N, int32_t V, int32_t mode, char* buf, size_t n) {
    if (S <= 0 || min_N < 0 || max_N < min_N || V < 1) return 0;
    const int m = align_mode(S, mode);
    const int P = split_parts(S, m, mode);
    int ids[kNumBuckets + 8];
    const int cnt = P > 1 ? buckets_for_split(min_N, max_N, P, split_launch_id(max_N, P), ids)
                          : buckets_for(min_N, max_N, m, ids);
    const int vs = V <= 32 ? 32 : (V <= 64 ? 64 : kGatherVS);
    size_t used = 0;
    for (int i = 0; i < cnt && buf && n > 0; ++i) {
        const int id = ids[i] & ~kSplitFlag;
        char one[160];
        if (ids[i] & kSplitFlag)
            snprintf(one, sizeof one, "%svoid wx::align_dp_split_kernel<%d, %d, %d>(wx::AlignArgs)", i ? ";" : "",
                     bucket_C(id), vs, bucket_W(id));
        else
            snprintf(one, sizeof one, "%svoid wx::align_dp_kernel<%d, %d, %d, %d>(wx::AlignArgs)", i ? ";" : "",
                     bucket_C(id), vs, bucket_W(id), id & 1);
        const size_t len = strlen(one);
        if (used + len + 1 > n) break;
        memcpy(buf + used, one, len + 1);
        used += len;
    }
    return cnt;
}

int wx_trellis(const float* em, const int64_t* em_off, int32_t V, const int32_t* tok, const int64_t* tok_off,
               const int32_t* blank_id, int32_t S, int64_t max_N, float* trellis, const int64_t* tr_off,
               void* stream) {
    if (S < 0 || max_N < 0) return WX_E_INVALID;
    if (S == 0) return WX_OK;
    if (!em || !em_off || !tok_off || !blank_id || !trellis || !tr_off) return WX_E_INVALID;
    if (V < 1 || V > WX_MAX_VOCAB) return WX_E_VOCAB;
#ifdef WX_DEV_V32
    if (V > 32) return WX_E_INVALID;  // development build: only the V <= 32 kernels exist
#endif
    if (max_N > WX_MAX_TOKENS) return WX_E_TOO_LONG;
    TrellisArgs a;
    a.em = em; a.em_off = em_off; a.V = V; a.tok = tok; a.tok_off = tok_off; a.blank_id = blank_id;
    a.tr = trellis; a.tr_off = tr_off;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    a.x4 = (V == 32 && (reinterpret_cast<uintptr_t>(em) & 15) == 0) ? 1 : 0;
    int ids[kNumBuckets];
    const int n = buckets_for(0, max_N, 0, ids);
    const dim3 grid(S);
    return fork_join(st, n, [&](int i, hipStream_t s) {
#define WX_LAUNCH_TR(CC, WW, HH)                                                                        \
        if (!HH && ids[i] == bucket_make(CC, WW, 0)) {                                                \
            if (V <= 32) launch_trellis<CC, 32, WW>(grid, s, a);                                         \
            else if (V <= 64) launch_trellis<CC, WX_VS64, WW>(grid, s, a);                               \
            else launch_trellis<CC, WX_VSG, WW>(grid, s, a);                                            \
        }
        WX_BUCKETS(WX_LAUNCH_TR)
#undef WX_LAUNCH_TR
    });
}

size_t wx_backtrack_workspace_bytes(int32_t S, int64_t sum_T, int64_t max_N) {
    Carver c{nullptr};
    BacktrackArgs a;
    return carve_backtrack(c, S, sum_T, max_N, a);
}

int wx_backtrack(const float* trellis, const int64_t* tr_off, const float* em, const int64_t* em_off, int32_t V,
                 const int32_t* tok, const int64_t* tok_off, const int32_t* blank_id, int32_t S, int64_t max_N,
                 int64_t sum_T, int32_t* path_tok, int32_t* path_time, float* path_prob, int32_t* path_len,
                 int32_t* t_start, void* workspace, size_t workspace_bytes, void* stream) {
    if (S < 0 || max_N < 0 || sum_T < 0) return WX_E_INVALID;
    if (S == 0) return WX_OK;
    if (!trellis || !tr_off || !em || !em_off || !tok_off || !blank_id || !path_tok || !path_time || !path_prob ||
        !path_len || !t_start || !workspace)
        return WX_E_INVALID;
    if (V < 1) return WX_E_VOCAB;
    BacktrackArgs a;
    Carver ws{workspace};
    if (workspace_bytes < carve_backtrack(ws, S, sum_T, max_N, a)) return WX_E_WORKSPACE;
    a.tr = trellis; a.tr_off = tr_off; a.em = em; a.em_off = em_off; a.V = V; a.tok = tok; a.tok_off = tok_off;
    a.blank_id = blank_id; a.path_tok = path_tok; a.path_time = path_time; a.path_prob = path_prob;
    a.path_len = path_len; a.t_start = t_start;
    hipLaunchKernelGGL(backtrack_kernel, dim3(S), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}

int wx_merge_repeats(const int32_t* path_tok, const int32_t* path_time, const float* path_prob,
                     const int64_t* path_off, const int32_t* path_len, int32_t S, int32_t* seg_tok,
                     int32_t* seg_start, int32_t* seg_end, double* seg_score, int32_t* seg_count, void* stream) {
    if (S < 0) return WX_E_INVALID;
    if (S == 0) return WX_OK;
    if (!path_tok || !path_time || !path_prob || !path_off || !path_len || !seg_tok || !seg_start || !seg_end ||
        !seg_score || !seg_count)
        return WX_E_INVALID;
    MergeArgs a;
    a.ptok = path_tok; a.ptime = path_time; a.pprob = path_prob; a.path_off = path_off; a.path_len = path_len;
    a.seg_tok = seg_tok; a.seg_start = seg_start; a.seg_end = seg_end; a.seg_score = seg_score;
    a.seg_count = seg_count;
    hipLaunchKernelGGL(merge_repeats_kernel, dim3(S), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}

int wx_column0_cumsum(const float* em, int64_t T, int32_t V, double* S, void* stream) {
    if (T < 0 || V < 1 || !S || (T > 0 && !em)) return WX_E_INVALID;
    hipLaunchKernelGGL(column0_cumsum_kernel, dim3(1), dim3(kWave), 0, reinterpret_cast<hipStream_t>(stream), em, T,
                       V, S);
    return launch_status();
}
}  // extern "C"

#ifdef WX_PHASE_TIMING
extern "C" int wx_debug_phases(unsigned long long* host, int n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(wx::wx_phase), sizeof(unsigned long long) * 6 * (size_t)n, 0,
                                    hipMemcpyDeviceToHost);
}
extern "C" int wx_debug_cq(unsigned long long* host, int n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(wx::wx_cq), sizeof(unsigned long long) * 48 * 3 * (size_t)n, 0,
                                    hipMemcpyDeviceToHost);
}
extern "C" int wx_debug_loop(unsigned long long* host, int n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(wx::wx_loop), sizeof(unsigned long long) * wx::kLoopSlots * 3 * (size_t)n, 0,
                                    hipMemcpyDeviceToHost);
}
#endif
